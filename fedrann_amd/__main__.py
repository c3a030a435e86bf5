"""`python -m fedrann_amd` -- the fedrann command line on the GPU hot path.

Keeps the reference's flags and defaults (fedrann/__main__.py:69-171) and its stage sequence
(run_fedrann_pipeline :302-391): k-mer counting / sampling / search (stage 1, on the GPU too) ->
projection matrix -> embeddings -> k-NN -> overlaps.tsv.  Entry points:

    -i reads.fa[.gz]                              the whole pipeline, like the reference
    -i reads.fa --kmer-library fwd_kmer_library.fasta          stage 1b on (search only)
    --kmer-searcher-output out/temp/kmer_searcher/output.bin --kmer-library out/temp/fwd_kmer_library.fasta
        (what the reference leaves behind with --keep-intermediates), or
    --feature-matrix feature_matrix.npz --kmer-counts counts.npy [--read-names names.txt]
        (scipy.sparse.save_npz binary CSR of the rows to search; see feature_extraction.py).

--no-projection: stages 2-3 build the IDF-weighted feature rows (value of feature f = idf[f]) instead of the
projection and the embeddings, and stage 4 searches them exactly (fdr_knn_sparse); -n is ignored.  Over several
--devices the user chooses what is divided, --sparse-shard targets (each rank indexes its own rows, the ranks exchange
query blocks and k candidates per query, fdr_topk_merge merges them) or queries (each rank indexes all rows and
searches its own); either way overlaps.tsv is the one-GPU file byte for byte.
--no-projection-metric jaccard (with --no-projection): stage 2 builds no weights and stage 4 searches the rows'
k-mer sets by exact Jaccard distance (fdr_knn_sparse_metric), the quantity MinHash tools estimate.
--no-projection-metric weighted_jaccard: stage 2 builds the IDF weights as for cosine (a negative weight, count > F,
becomes 0) and stage 4 searches the weighted rows by exact weighted Jaccard (Ruzicka) distance.
--no-projection-radius R (with --no-projection, any metric): instead of k neighbours, stage 4 writes every read within
distance R of each read (0 <= R < 1; fdr_sparse_index_radius_search), a block of rows at a time.  Over several
--devices only with --sparse-shard targets: each rank indexes its own rows, the ranks exchange query blocks and the
ragged rows of hits, fdr_radius_merge merges them, and overlaps.tsv is the one-GPU file byte for byte.
--radius R (the default, projected mode, one GPU, -n <= 512): stage 4 embeds the rows once, keeps them on the device
(fdr_dense_index_embed) and writes every read within cosine distance R of each read (0 <= R < 1;
fdr_dense_index_radius_search), a block of rows at a time; --nndescent-n-neighbors is ignored.
--rescore METRIC (the default, projected mode, one GPU): stage 4 takes --rescore-candidates K' >= k neighbours per read
from the projected search, scores exactly those pairs on the feature rows under METRIC (fdr_sparse_rescore: the
distances of --no-projection --no-projection-metric METRIC, bit for bit) and writes the best k with them.
--radius R --radius-rescore METRIC [--radius-rescore-bound R2]: the candidates of the projected radius search, every
pair scored exactly on the feature rows under METRIC (the rows go to the device once: fdr_rescore_rows_build), cut at
R2 in that metric (default 1: every projected hit is kept) and written in the exact order (fdr_rescore_rows_radius).
--refine METRIC [--refine-fan F] [--refine-rounds T] [--refine-reverse] (the default, projected mode, one GPU, after
--rescore where that is given): the feature rows go to the device once (fdr_rescore_rows_build) and T rounds of
refinement run on the lists: a read's candidates are its F nearest neighbours and theirs (fdr_graph_expand), scored
exactly under METRIC and cut to the best k (fdr_rescore_rows_refine); round i's graph is round i - 1's rows.
--symmetrize union|mutual (any of the one-GPU modes above): the graph the mode is about to write is symmetrised on the
GPU first (fdr_graph_symmetrize: a pair under both reads when either lists the other, or only where each lists the
other, at the smaller distance) and written once through fdr_overlaps_write_csr; the radius modes collect their row
blocks on the host before that.  Refused over several --devices.
--components union|mutual [--components-distance D] (the same one-GPU modes): components.tsv beside overlaps.tsv, the
connected components of the rows as searched, before any --symmetrize (fdr_graph_components: two reads are joined when
either lists the other, or only where each lists the other, at a distance <= D; by default every listed pair joins).
One line per read in row order: read_name, orientation, component (numbered by their first read), component_size.
overlaps.tsv is what the run writes without the flag, byte for byte; the radius modes collect their row blocks on the
host as for --symmetrize.  Refused over several --devices.

--devices 0,1,...: every stage is sharded over several GPUs of the node.  The parent process starts one
child per GPU BEFORE it touches a GPU itself; from reads, every child counts and searches its byte range of
the file (stage1_sharded.py), then embeds its row block, the blocks are all-gathered (RCCL), every child
searches its rows against all rows and writes its part of overlaps.tsv; the parent concatenates the parts in
rank order (byte-identical to the single-GPU file).  With --no-projection the children run the sparse search under
--sparse-shard instead of the embed / all-gather / search.
"""
import argparse
import logging
import os
from os.path import abspath, join
import subprocess
import sys
from shutil import copyfileobj, rmtree
from typing import List

import numpy as np
import pandas as pd

from . import __description__, __version__
from . import global_variables
from .feature_extraction import (build_feature_csr, embed_csr, get_feature_matrix, get_metadata,
                                 load_feature_matrix_npz, save_feature_matrix_npz)
from .nearest_neighbors import NNDescent_ava
from .precompute import build_precompute_matrix, get_precompute_matrix, idf_weights

LOG_FORMAT = "%(asctime)s - %(levelname)s - %(message)s"  # custom_logging.py:8
logger = logging.getLogger("fedrann_amd")
logger.setLevel(logging.DEBUG)


def _setup_logging(logfile=None):
    if not logger.handlers:
        h = logging.StreamHandler()
        h.setFormatter(logging.Formatter(LOG_FORMAT))
        logger.addHandler(h)
    if logfile:
        fh = logging.FileHandler(logfile)
        fh.setFormatter(logging.Formatter(LOG_FORMAT))
        logger.addHandler(fh)


def build_parser():
    from ._lib import FDR_MAX_K
    p = argparse.ArgumentParser(prog="fedrann", description=__description__,
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("-i", "--input", type=str, required=False, default=None,
                   help="Path to the input FASTQ/FASTA file (needs the reference's stage-1 tools; "
                        "use --kmer-searcher-output or --feature-matrix instead).")
    p.add_argument("-o", "--output-dir", type=str, required=True, help="Directory to save output files.")
    p.add_argument("-k", "--kmer-size", type=int, default=16, help="K-mer size for feature extraction.")
    p.add_argument("--kmer-sample-fraction", type=float, default=0.005,
                   help="Percentage of k-mer used to build feature matrix.")
    p.add_argument("--kmer-min-multiplicity", type=int, default=2,
                   help="Minimum allowed frequency of a k-mer in all reads.")
    p.add_argument("--threads", type=int, default=1)
    p.add_argument("--chunk-size", type=int, default=1000)
    p.add_argument("-n", "--embedding-dimension", type=int, default=500)
    p.add_argument("--nndescent-n-trees", type=int, default=300, help="Number of trees to use in NNDescent.")
    p.add_argument("--nndescent-n-neighbors", type=int, default=50,
                   help="Number of neighbors to use in building NNDescent index.")
    p.add_argument("--seed", type=int, default=356115, help="Random seed for reproducibility.")
    p.add_argument("--save-feature-matrix", action="store_true", default=False,
                   help="Save the feature matrix to a file.")
    p.add_argument("--keep-intermediates", action="store_true", default=False,
                   help="Do not remove intermediate files")
    p.add_argument("--mprof", action="store_true", default=False, help="Record memory usage.")
    g = p.add_argument_group("hot-path entry points (GPU build)")
    g.add_argument("--kmer-searcher-output", type=str, default=None,
                   help="kmer_searcher output.bin (reference intermediate temp/kmer_searcher/output.bin).")
    g.add_argument("--kmer-library", type=str, default=None,
                   help="fwd_kmer_library.fasta (jellyfish dump with counts) for the IDF weights.")
    g.add_argument("--feature-matrix", type=str, default=None,
                   help="feature_matrix.npz: binary read x feature CSR (scipy.sparse.save_npz).")
    g.add_argument("--kmer-counts", type=str, default=None,
                   help="With --feature-matrix: .npy of forward-library counts (int, length F/2) or a "
                        "fwd_kmer_library.fasta.")
    g.add_argument("--read-names", type=str, default=None,
                   help="With --feature-matrix: text file, one 'name<TAB>strand' (or just name) per row.")
    g.add_argument("--no-projection", action="store_true", default=False,
                   help="Search the IDF-weighted feature rows themselves (exact cosine k-NN, no random projection: "
                        "the ground truth the projection approximates); -n is ignored.  Over several --devices: "
                        "see --sparse-shard.")
    g.add_argument("--no-projection-metric", choices=["cosine", "jaccard", "weighted_jaccard"], default="cosine",
                   help="With --no-projection: cosine on the IDF-weighted rows, the exact Jaccard distance of the "
                        "rows' feature sets (no weights), or the exact weighted Jaccard distance of the IDF-weighted "
                        "rows (sum of minima over sum of maxima; a negative IDF counts as 0).")
    g.add_argument("--sparse-shard", choices=["targets", "queries"], default=None,
                   help="With --no-projection and several --devices (required there): what the ranks divide.  targets: "
                        "a rank loads and indexes only its own rows (1 / ranks of the index memory and of the build), "
                        "sees every query and the ranks exchange k candidates per query; needs k <= the rows of every "
                        "rank (with --no-projection-radius: every hit per query, and at least one row on every rank).  "
                        "queries: every rank loads and indexes all rows and searches its own; nothing is "
                        "exchanged.")
    g.add_argument("--device", type=int, default=None, help="GPU ordinal (default $LOCAL_RANK or 0).")
    g.add_argument("--no-projection-radius", type=float, default=None, metavar="R",
                   help="With --no-projection: instead of the k nearest rows, write every row within distance R of "
                        "each read (0 <= R < 1, under the --no-projection-metric; exact).  overlaps.tsv then holds "
                        "as many lines per read as it has such neighbours, ranked by distance; "
                        "--nndescent-n-neighbors is ignored.  One GPU, or several --devices with --sparse-shard targets "
                        "(the ranks' rows of hits are merged exactly: the same file).")
    g.add_argument("--radius", type=float, default=None, metavar="R",
                   help="In the default, projected mode: instead of the k nearest rows, write every row within cosine "
                        "distance R of each read (0 <= R < 1: the distances the k-NN search reports).  overlaps.tsv "
                        "then holds as many lines per read as it has such neighbours, ranked by distance; "
                        "--nndescent-n-neighbors is ignored.  One GPU only, -n up to 512.  With --no-projection: "
                        "--no-projection-radius.")
    g.add_argument("--rescore", choices=["cosine", "jaccard", "weighted_jaccard"], default=None,
                   help="In the default, projected mode: search the projected rows for --rescore-candidates neighbours "
                        "per read, score exactly those pairs on the feature rows under this metric (the distances "
                        "--no-projection --no-projection-metric reports, bit for bit) and write the best "
                        "--nndescent-n-neighbors of them with the exact distances.  One GPU; not with --radius or "
                        "--no-projection (whose distances are exact already).")
    g.add_argument("--rescore-candidates", type=int, default=None, metavar="K'",
                   help="With --rescore: candidates per read taken from the projected search, k <= K' <= min(%d, reads) "
                        "with k = --nndescent-n-neighbors; by default max(k, min(2 k, 64)), capped by the number of "
                        "reads.  K' > 64 takes the projected search off its fp16 prefilter (DESIGN.md section 10): a "
                        "cost cliff, not a slope." % FDR_MAX_K)
    g.add_argument("--radius-rescore", choices=["cosine", "jaccard", "weighted_jaccard"], default=None,
                   help="With --radius: score every (read, projected hit) pair on the feature rows under this metric "
                        "(the distances --no-projection --no-projection-metric reports, bit for bit), keep the pairs "
                        "within --radius-rescore-bound and write them with the exact distances, ranked by them.  One "
                        "GPU; not with --no-projection.")
    g.add_argument("--radius-rescore-bound", type=float, default=None, metavar="R2",
                   help="With --radius-rescore: the bound in the exact metric, 0 <= R2 <= 1; by default 1, which keeps "
                        "every hit of the projected radius search.")
    g.add_argument("--refine", choices=["cosine", "jaccard", "weighted_jaccard"], default=None,
                   help="In the default, projected mode, after the search (and --rescore, whose metric must then be "
                        "the same): refine every read's list among the neighbours of its neighbours.  The candidates "
                        "of a read are its --refine-fan nearest entries and theirs (fdr_graph_expand), scored on the "
                        "feature rows under this metric (the distances --no-projection --no-projection-metric "
                        "reports, bit for bit) and cut to the best --nndescent-n-neighbors "
                        "(fdr_rescore_rows_refine): the exact-metric route to candidates the projection did not "
                        "name, without widening --rescore-candidates past 64.  One GPU; not with --radius or "
                        "--no-projection.")
    g.add_argument("--refine-fan", type=int, default=None, metavar="F",
                   help="With --refine: entries of a list that are followed, 1 <= F <= %d; by default "
                        "min(--nndescent-n-neighbors, %d).  A read has at most F + F^2 candidates a round." % (FDR_MAX_K, FDR_MAX_K))
    g.add_argument("--refine-rounds", type=int, default=None, metavar="T",
                   help="With --refine: rounds, each on the rows the round before it left; by default 1.")
    g.add_argument("--refine-reverse", action="store_true", default=False,
                   help="With --refine: each round first takes the union graph (fdr_graph_symmetrize), so that the "
                        "reads that list a read are followed too (NN-descent's reverse neighbours).")
    g.add_argument("--symmetrize", choices=["union", "mutual"], default=None,
                   help="Symmetrise the neighbour graph on the GPU before overlaps.tsv is written "
                        "(fdr_graph_symmetrize): union lists a pair under both reads when either read lists the other, "
                        "mutual keeps a pair only where each read lists the other; the smaller of the two distances, "
                        "every read's row ranked by distance.  Applies to what one GPU is about to write, in every "
                        "one-GPU mode (k-NN, --no-projection, --rescore, --radius, --no-projection-radius, "
                        "--radius-rescore); the radius modes collect their row blocks on the host first (16 bytes a "
                        "hit) and are refused at 2^31 hits.  Refused over several --devices: a rank holds only its "
                        "own rows' lists, while a reverse entry can come from any row.")
    g.add_argument("--components", choices=["union", "mutual"], default=None,
                   help="Write components.tsv beside overlaps.tsv: the connected components of the neighbour graph as "
                        "searched (before any --symmetrize), found on the GPU (fdr_graph_components).  union joins two "
                        "reads when either lists the other, mutual only where each lists the other.  One line per "
                        "read: read_name, orientation, component (numbered by their first read), component_size.  "
                        "overlaps.tsv is the file the run writes without this flag.  In every one-GPU mode that "
                        "--symmetrize serves; the radius modes collect their row blocks on the host as for "
                        "--symmetrize.  Refused over several --devices.")
    g.add_argument("--components-distance", type=float, default=None, metavar="D",
                   help="With --components: join only pairs at distance <= D (mutual: the smaller of the two "
                        "directions); by default every listed pair joins.  D >= 0.")
    g.add_argument("--devices", type=str, default=None,
                   help="Comma-separated GPU ordinals: shard the rows over these GPUs (one process each).")
    g.add_argument("--dist-backend", choices=["nccl", "gloo"], default="nccl",
                   help="With --devices: nccl (= RCCL over xGMI; one GPU per process) or gloo (processes may "
                        "share a GPU: one-GPU rehearsal of the sharded path).")
    g.add_argument("--rank-worker", action="store_true", default=False, help=argparse.SUPPRESS)
    g.add_argument("--stage1-cuts", type=str, default=None, help=argparse.SUPPRESS)
    return p


def parse_command_line_arguments(argv=None):
    return build_parser().parse_args(argv)


def get_neighbors_ava(embedding_matrix, nndescent_n_trees, nndescent_n_neighbors, leaf_size=200):
    """Same call shape as the reference (__main__.py:174-199)."""
    logger.info("Using exact GPU k-NN in place of NNDescent (n_trees = %s, leaf_size = %s are inert)",
                nndescent_n_trees, leaf_size)
    return NNDescent_ava().get_neighbors(
        embedding_matrix, metric="cosine", index_n_neighbors=nndescent_n_neighbors,
        n_trees=nndescent_n_trees, leaf_size=leaf_size, n_iters=None, diversify_prob=1.0,
        pruning_degree_multiplier=1.5, low_memory=True, n_jobs=global_variables.threads,
        seed=global_variables.seed, verbose=True)


def get_output_dataframe(neighbor_matrix, neighbor_distances, read_names: List[str],
                         strands: List[int]) -> pd.DataFrame:
    """Vectorised equivalent of the reference's N x k Python loop (__main__.py:261-300).

    Same rows in the same order with the same dtypes: a neighbour is skipped only when it is the
    query row itself; neighbor_rank keeps the column number; the distance column is float32 (pandas
    prints its shortest repr); a negative index aliases from the end like Python indexing does.
    """
    idx = np.asarray(neighbor_matrix)
    dist = np.asarray(neighbor_distances)
    n = idx.shape[0]
    names = np.asarray(read_names, dtype=object)
    orient = np.where(np.asarray(strands, dtype=np.int64) == 0, "+", "-").astype(object)
    keep = idx != np.arange(n, dtype=idx.dtype)[:, None]
    q, r = np.nonzero(keep)  # row-major = the loop's order
    t = idx[q, r]
    columns = {
        "query_name": names[q],
        "query_orientation": orient[q],
        "target_name": names[t],
        "target_orientation": orient[t],
        "neighbor_rank": r.astype(np.int64),
        "distance": dist[q, r],
    }
    df = pd.DataFrame(columns)
    logger.debug("Output DataFrame shape: %s", df.shape)
    return df


def write_overlaps(path, neighbor_matrix, distances, read_names, strands, row0=0, header=True):
    """overlaps.tsv through the native writer (fdr_overlaps_write): the bytes get_output_dataframe(...)
    .to_csv(path, sep="\\t", index=False) produces (__main__.py:261-300, :385), without the DataFrame.
    neighbor_matrix / distances may be the rows row0.. of the graph (a rank's block); read_names / strands
    describe all rows.  Returns the number of data lines."""
    from . import _lib
    name_off, names = _lib.pack_names(read_names)
    return _lib.overlaps_write(path, np.asarray(neighbor_matrix), np.asarray(distances), name_off, names,
                               np.asarray(strands, dtype=np.uint8), row0=row0, header=header,
                               n_threads=global_variables.threads if global_variables.threads > 1 else 0)


RADIUS_BLOCK_ROWS = 1 << 16  # query rows per radius_search call of --no-projection-radius and --radius
RADIUS_MAX_HITS = 1 << 26    # ... and the cap on the hits of one device call (8 bytes held, 8 of scratch, 8 on the host;
                             # --radius: on its fp16 candidates, 16 bytes each)


def check_radius(args, flag, r, needs_no_projection):
    """A radius option (`flag`, its value r; None: not given) against the other options, before any work:
    --no-projection-radius needs --no-projection, --radius refuses it and is bound to the fp16 passes' dimensions.  Over
    several --devices only --no-projection-radius with --sparse-shard targets runs (distributed.sparse_radius_sharded)."""
    if r is None:
        return
    if needs_no_projection and not args.no_projection:
        raise SystemExit("--no-projection-radius needs --no-projection (the projected search has no radius form)")
    if not needs_no_projection and args.no_projection:
        raise SystemExit("--radius is the projected search's; with --no-projection use --no-projection-radius")
    if not 0.0 <= np.float32(r) < 1.0:  # (NaN fails both)
        raise SystemExit("%s must be in [0, 1), got %r (every read is within 1 of every other)" % (flag, r))
    if len(device_list(args.devices)) > 1:
        if not needs_no_projection:
            raise SystemExit("--radius runs on one GPU: the projected radius search is not sharded over --devices")
        if args.sparse_shard != "targets":
            raise SystemExit("--no-projection-radius runs on one GPU, or over --devices with the targets divided: "
                             "give --sparse-shard targets (%s)"
                             % ("--sparse-shard queries has no radius form" if args.sparse_shard
                                else "without --sparse-shard nothing says what to divide"))
    from . import _lib
    if not needs_no_projection and args.embedding_dimension > _lib.FDR_FAST_MAX_DIM:
        raise SystemExit("--radius needs -n/--embedding-dimension <= %d, the reach of the fp16 passes (got %d)"
                         % (_lib.FDR_FAST_MAX_DIM, args.embedding_dimension))


def default_rescore_candidates(k, n=None):
    """K' of --rescore where --rescore-candidates is not given: twice k while that stays on the projected search's
    fp16 prefilter (K' <= 64), never below k, and no more than the n reads there are."""
    kp = max(k, min(2 * k, 64))
    return kp if n is None else min(kp, n)


def check_rescore(args):
    """--rescore / --rescore-candidates against the other options, before any work.  Returns K' (None without
    --rescore); that K' <= the number of reads can only be checked once they are loaded (run_fedrann_pipeline)."""
    from . import _lib
    if args.rescore is None:
        if args.rescore_candidates is not None:
            raise SystemExit("--rescore-candidates needs --rescore (without it nothing is re-scored)")
        return None
    if args.no_projection:
        raise SystemExit("--rescore is the projected search's second stage; the distances of --no-projection are exact "
                         "already")
    if args.radius is not None:
        raise SystemExit("--rescore re-scores k-NN lists: it does not run with --radius (a radius in the exact metric "
                         "is --no-projection-radius)")
    if len(device_list(args.devices)) > 1:
        raise SystemExit("--rescore runs on one GPU: over --devices a rank holds only its own rows of the feature "
                         "matrix, and a candidate may be any row")
    k = args.nndescent_n_neighbors
    kp = default_rescore_candidates(k) if args.rescore_candidates is None else args.rescore_candidates
    if not k <= kp <= _lib.FDR_MAX_K:
        raise SystemExit("--rescore-candidates must be in [--nndescent-n-neighbors = %d, %d], got %d"
                         % (k, _lib.FDR_MAX_K, kp))
    return kp


def check_refine(args):
    """--refine and its options against the other options, before any work.  Returns (fan or None, rounds); (None, 0)
    without --refine."""
    from . import _lib
    if args.refine is None:
        for flag, given in (("--refine-fan", args.refine_fan is not None), ("--refine-rounds", args.refine_rounds is not None),
                            ("--refine-reverse", args.refine_reverse)):
            if given:
                raise SystemExit("%s needs --refine (without it nothing is refined)" % flag)
        return None, 0
    if args.no_projection:
        raise SystemExit("--refine refines the projected search's lists: it does not run with --no-projection, whose "
                         "lists are exact already")
    if args.radius is not None:
        raise SystemExit("--refine refines k-NN lists: it does not run with --radius")
    if len(device_list(args.devices)) > 1:
        raise SystemExit("--refine runs on one GPU: over --devices a rank holds only its own rows of the feature "
                         "matrix, and a candidate may be any row")
    if args.rescore is not None and args.rescore != args.refine:
        raise SystemExit("--refine %s after --rescore %s: the two metrics must be the same (the refinement follows "
                         "the re-scored distances)" % (args.refine, args.rescore))
    if args.refine_fan is not None and not 1 <= args.refine_fan <= _lib.FDR_MAX_K:
        raise SystemExit("--refine-fan must be in [1, %d], got %d" % (_lib.FDR_MAX_K, args.refine_fan))
    rounds = 1 if args.refine_rounds is None else args.refine_rounds
    if rounds < 1:
        raise SystemExit("--refine-rounds must be at least 1, got %d" % rounds)
    return args.refine_fan, rounds


def check_radius_rescore(args):
    """--radius-rescore / --radius-rescore-bound against the other options, before any work.  Returns R2 (None without
    --radius-rescore).  What --radius itself refuses (--no-projection, several --devices, -n > 512) is check_radius's;
    they are named here too, so that the message speaks of the flag that was given."""
    if args.radius_rescore is None:
        if args.radius_rescore_bound is not None:
            raise SystemExit("--radius-rescore-bound needs --radius-rescore (without it nothing is re-scored)")
        return None
    if args.no_projection:
        raise SystemExit("--radius-rescore is the projected radius search's second stage; the distances of "
                         "--no-projection-radius are exact already")
    if args.radius is None:
        raise SystemExit("--radius-rescore needs --radius (it re-scores the projected radius search's hits)")
    if len(device_list(args.devices)) > 1:
        raise SystemExit("--radius-rescore runs on one GPU: the projected radius search is not sharded over --devices")
    r2 = 1.0 if args.radius_rescore_bound is None else args.radius_rescore_bound
    if not 0.0 <= np.float32(r2) <= 1.0:  # (NaN fails both)
        raise SystemExit("--radius-rescore-bound must be in [0, 1], got %r" % (r2,))
    return r2 + 0.0  # (-0.0 is 0)


class RescoredRadius:
    """write_radius_overlaps' index of --radius-rescore: radius_search(radius, lo, hi, max_hits=) is the dense index's,
    its rows then re-scored on `rows` (a RescoreRows of the same reads) and cut at `bound` in the exact metric."""

    def __init__(self, index, rows, bound):
        self.index, self.rows, self.bound, self.n = index, rows, bound, index.n
        self.candidates = 0  # the projected hits so far

    def radius_search(self, radius, lo, hi, max_hits):
        ip, idx, _ = self.index.radius_search(radius, lo, hi, max_hits=max_hits)
        self.candidates += int(ip[-1])
        return self.rows.radius(ip, idx, self.bound, q_lo=lo, max_entries=max_hits)


def check_symmetrize(args):
    """--symmetrize against the other options, before any work: one GPU only."""
    if args.symmetrize is not None and len(device_list(args.devices)) > 1:
        raise SystemExit("--symmetrize runs on one GPU: over --devices a rank holds only its own rows' lists, and a "
                         "reverse entry can come from any row")


def check_components(args):
    """--components / --components-distance against the other options, before any work: one GPU only, the distance
    only with the flag, and neither negative nor NaN."""
    if args.components_distance is not None:
        if args.components is None:
            raise SystemExit("--components-distance needs --components union|mutual")
        if np.isnan(args.components_distance) or np.signbit(args.components_distance):  # (-0.0 too: bits decide)
            raise SystemExit("--components-distance must be a distance >= 0, got %r" % args.components_distance)
    if args.components is not None and len(device_list(args.devices)) > 1:
        raise SystemExit("--components runs on one GPU: over --devices a rank holds only its own rows' lists, and a "
                         "reverse entry can come from any row")


def write_components(path, ctx, graph, mode, max_distance, read_names, strands):
    """components.tsv of `graph` ((idx [n, k], dist [n, k]) or a ragged triple, every row of the graph):
    Context.graph_components, then one line per row in row order: read_name, orientation (+ / - from the strand, as in
    overlaps.tsv), component, component_size.  Returns the number of components."""
    labels, sizes = ctx.graph_components(graph, mode=mode, max_distance=max_distance)
    logger.info("--components %s: %d components of %d rows, the largest of %d, %d singletons", mode, sizes.size,
                labels.size, int(sizes.max()), int(np.sum(sizes == 1)))
    orient = np.where(np.asarray(strands, dtype=np.int64) == 0, "+", "-")
    of_row = sizes[labels]
    with open(path, "w") as f:
        f.write("read_name\torientation\tcomponent\tcomponent_size\n")
        f.writelines("%s\t%s\t%d\t%d\n" % (read_names[r], orient[r], labels[r], of_row[r]) for r in range(labels.size))
    return int(sizes.size)


def _gathered(blocks):
    """the ragged graph of a radius search's row blocks, in row order"""
    starts = np.cumsum([0] + [int(b[0][-1]) for b in blocks[:-1]])
    indptr = np.concatenate([np.zeros(1, np.int64)] + [b[0][1:] + s for b, s in zip(blocks, starts)])
    return indptr, np.concatenate([b[1] for b in blocks]), np.concatenate([b[2] for b in blocks])


def write_symmetrized(path, ctx, graph, mode, read_names, strands):
    """overlaps.tsv of the union / mutual rows of `graph` ((idx [n, k], dist [n, k]) or a ragged triple, every row of
    the graph): Context.graph_symmetrize, then one fdr_overlaps_write_csr.  Returns the data lines."""
    from . import _lib
    ip, idx, dist = ctx.graph_symmetrize(graph, mode=mode, max_entries=2 ** 31 - 1)
    logger.info("--symmetrize %s: %d entries of %d rows became %d", mode, graph[-2].size, ip.size - 1, int(ip[-1]))
    name_off, names = _lib.pack_names(read_names)
    return _lib.overlaps_write_csr(path, ip, idx, dist, name_off, names, np.asarray(strands, dtype=np.uint8),
                                   n_threads=global_variables.threads if global_variables.threads > 1 else 0)


def write_radius_overlaps(path, index, radius, read_names, strands, block_rows=None, max_hits=None, symmetrize=None,
                          ctx=None, components=None):
    """overlaps.tsv of a radius search of all rows of `index` (a SparseIndex or a DenseIndex: both have n and
    radius_search(radius, lo, hi, max_hits=)), a block of rows at a time: each block's ragged result
    is appended through fdr_overlaps_write_csr, so the host holds one block's hits.  block_rows / max_hits = None:
    RADIUS_BLOCK_ROWS / RADIUS_MAX_HITS as they stand at the call.  symmetrize ("union" / "mutual", with the Context
    ctx): the blocks are collected on the host instead (16 bytes a hit; 2^31 hits or more are refused), symmetrised in
    one piece and written once (write_symmetrized).  components ((mode, max_distance), with ctx): the blocks are
    collected in the same way, under the same refusal, and components.tsv of the rows as searched is written beside
    `path` (write_components); without symmetrize the blocks are still appended as they come, so overlaps.tsv is the
    unflagged run's.  Returns the data lines."""
    from . import _lib
    block_rows = RADIUS_BLOCK_ROWS if block_rows is None else block_rows
    max_hits = RADIUS_MAX_HITS if max_hits is None else max_hits
    collect = symmetrize is not None or components is not None
    name_off, names = _lib.pack_names(read_names)
    strand_codes = np.asarray(strands, dtype=np.uint8)
    threads = global_variables.threads if global_variables.threads > 1 else 0
    blocks, total, lines = [], 0, 0
    for lo in range(0, index.n, block_rows):
        hi = min(index.n, lo + block_rows)
        ip, idx, dist = index.radius_search(radius, lo, hi, max_hits=max_hits)
        if collect:
            blocks.append((ip, idx, dist))
            total += int(ip[-1])
            if total >= 2 ** 31:
                if symmetrize is not None:
                    raise SystemExit("--symmetrize: the radius search has found %d hits by row %d, and a graph of 2^31 "
                                     "entries or more cannot be symmetrised: lower the radius" % (total, hi))
                raise SystemExit("--components: the radius search has found %d hits by row %d, and a graph of 2^31 "
                                 "entries or more cannot be labelled: lower the radius" % (total, hi))
        if symmetrize is None:
            lines += _lib.overlaps_write_csr(path, ip, idx, dist, name_off, names, strand_codes, row0=lo, append=lo > 0,
                                             header=lo == 0, n_threads=threads)
        logger.debug("radius search: rows [%d, %d), %d hits", lo, hi, int(ip[-1]))
    if not collect:
        return lines
    graph = _gathered(blocks)
    del blocks
    if components is not None:
        write_components(join(os.path.dirname(path), "components.tsv"), ctx, graph, components[0], components[1],
                         read_names, strands)
    if symmetrize is not None:
        lines = write_symmetrized(path, ctx, graph, symmetrize, read_names, strands)
    return lines


def _load_counts(path):
    if path.endswith(".npy"):
        return np.load(path).astype(np.int64)
    from .precompute import read_kmer_counts
    return read_kmer_counts(path)


def _load_names(path, nrows):
    if path is None:
        return ["row_%d" % i for i in range(nrows)], [0] * nrows
    names, strands = [], []
    with open(path) as f:
        for line in f:
            parts = line.rstrip("\n").split("\t")
            names.append(parts[0])
            strands.append(int(parts[1]) if len(parts) > 1 and parts[1] != "" else 0)
    if len(names) != nrows:
        raise ValueError("%s has %d lines, the feature matrix has %d rows" % (path, len(names), nrows))
    return names, strands


def check_limits(embedding_dimension, nndescent_n_neighbors):
    """The k-NN kernels' limits, checked before any work is done (the reference accepts any value)."""
    from . import _lib
    if not 1 <= embedding_dimension <= _lib.FDR_MAX_DIM:
        raise SystemExit("-n/--embedding-dimension must be in 1..%d for the GPU k-NN kernels (got %d)"
                         % (_lib.FDR_MAX_DIM, embedding_dimension))
    if not 1 <= nndescent_n_neighbors <= _lib.FDR_MAX_K:
        raise SystemExit("--nndescent-n-neighbors must be in 1..%d for the GPU k-NN kernels (got %d)"
                         % (_lib.FDR_MAX_K, nndescent_n_neighbors))


SPARSE_QUERY_BLOCK_ROWS = 1 << 16  # query rows per call of a sharded sparse search: bounds the device's result buffers


def device_list(devices):
    """The ordinals of --devices (None or empty: none)."""
    return [int(x) for x in (devices or "").split(",") if x.strip() != ""]


def check_sparse_shard(args):
    """--no-projection, --devices and --sparse-shard against each other, before any work: dividing a sparse search has
    two costs to choose between (a replicated index, or every query on every rank plus an exchange), so over several
    GPUs the user chooses."""
    several = len(device_list(args.devices)) > 1
    if args.sparse_shard and not args.no_projection:
        raise SystemExit("--sparse-shard %s needs --no-projection (the projected search shards its rows by itself)"
                         % args.sparse_shard)
    if args.sparse_shard and not several:
        raise SystemExit("--sparse-shard %s needs --devices with at least two GPUs (on one GPU there is nothing to "
                         "divide)" % args.sparse_shard)
    if args.no_projection and several and not args.sparse_shard:
        raise SystemExit("--no-projection with --devices over several GPUs needs to know what to divide: the index "
                         "(1 / ranks of its memory per GPU, candidates exchanged) or the queries (the whole index on "
                         "every GPU, nothing exchanged); choose with --sparse-shard targets|queries")


def sparse_weights(counts, n_features, metric):
    """Stage 2 of --no-projection: the feature weights that take the projection's place, float32 [n_features].  The IDF
    weights for metric="cosine"; clamped at 0 for "weighted_jaccard" (a feature with count > n_features has a negative
    IDF); None for "jaccard" (sets have no weights).  A row's values are weights[indices]."""
    if metric == "jaccard":
        return None
    w = idf_weights(counts, n_features)
    if metric == "weighted_jaccard":
        negative = int(np.count_nonzero(w < 0))
        logger.info("weighted Jaccard takes weights >= 0: %d of %d features have a negative IDF (count > %d) and "
                    "carry weight 0", negative, n_features, n_features)
        w = np.maximum(w, np.float32(0))
    return w


def load_inputs(*, output_dir, embedding_dimension, save_feature_matrix, kmer_searcher_output=None,
                kmer_library=None, feature_matrix=None, kmer_counts=None, read_names_path=None, save=True,
                no_projection=False, metric="cosine"):
    """Stages 2-3a of the reference pipeline on the host (__main__.py:329-345): the projection matrix and
    the read x feature CSR.  Returns (indptr, indices, n_features, P, read_names, strands); with no_projection the
    IDF weights of the features (float32 [n_features]) take P's place, or None with metric="jaccard" (sets have
    no weights); with metric="weighted_jaccard" the weights are clamped at 0 (a feature with count > n_features)."""
    jaccard = no_projection and metric == "jaccard"
    if jaccard:
        logger.info("--- 2. (skipped) no IDF weights: the Jaccard search takes the feature sets, values=None ---")
    if kmer_searcher_output:
        from .precompute import read_kmer_counts
        n_features = 2 * int(read_kmer_counts(kmer_library).size)  # (count_kmers.py:148)
        if jaccard:
            P = None
        elif no_projection:
            logger.info("--- 2. Generate IDF weights (no projection) ---")
            P = sparse_weights(read_kmer_counts(kmer_library), n_features, metric)
        else:
            logger.info("--- 2. Generate dimension reduction and IDF matrix ---")
            P, n_features = get_precompute_matrix(n_components=embedding_dimension, counter_file=kmer_library,
                                                  n_features=n_features)
        logger.info("--- 3. Generate feature matrix ---")
        indptr, indices, read_names, strands = build_feature_csr(kmer_searcher_output, n_features)
    else:
        indptr, indices, n_features = load_feature_matrix_npz(feature_matrix)
        counts = _load_counts(kmer_counts)
        if jaccard:
            P = None
        elif no_projection:
            logger.info("--- 2. Generate IDF weights (no projection) ---")
            P = sparse_weights(counts, n_features, metric)
        else:
            logger.info("--- 2. Generate dimension reduction and IDF matrix ---")
            P = build_precompute_matrix(counts, embedding_dimension, n_features=n_features)
        logger.info("--- 3. Generate feature matrix ---")
        read_names, strands = _load_names(read_names_path, indptr.size - 1)
    if save_feature_matrix and save:
        save_feature_matrix_npz(join(output_dir, "feature_matrix.npz"), indptr, indices, n_features)
    return indptr, indices, n_features, P, read_names, strands


def run_fedrann_pipeline(*, output_dir, embedding_dimension, nndescent_n_trees,
                         nndescent_n_neighbors, save_feature_matrix, keep_intermediates, chunk_size,
                         kmer_searcher_output=None, kmer_library=None, feature_matrix=None,
                         kmer_counts=None, read_names_path=None, no_projection=False,
                         no_projection_metric="cosine", no_projection_radius=None, radius=None, rescore=None,
                         rescore_candidates=None, radius_rescore=None, radius_rescore_bound=None, symmetrize=None,
                         components=None, refine=None, refine_fan=None, refine_rounds=1, refine_reverse=False):
    """Stages 2-4 of the reference pipeline (__main__.py:329-391) on one GPU.  The embeddings never leave
    HBM between the projection and the search (fdr_embed_knn), and only the features P has entries for
    cross PCIe (fdr_csr_compact; the saved feature_matrix.npz is the full matrix).  no_projection: stage 4
    searches the IDF-weighted feature rows themselves (value of feature f = idf[f]; fdr_knn_sparse), or with
    no_projection_metric="jaccard" their sets by Jaccard distance, with "weighted_jaccard" the rows with the IDF
    weights clamped at 0 by weighted Jaccard distance (both fdr_knn_sparse_metric).  no_projection_radius: stage 4
    builds the sparse index and writes every row within that distance of each read (fdr_sparse_index_radius_search)
    in row blocks, instead of k neighbours.  radius (projected mode): stage 4 embeds once into the context's dense
    index (fdr_dense_index_embed) and writes every row within that cosine distance of each read
    (fdr_dense_index_radius_search) in row blocks.  rescore (projected mode, a sparse metric's name): stage 4 searches
    the projected rows for rescore_candidates neighbours per read (None: default_rescore_candidates), scores those pairs
    on the feature rows with the values --no-projection gives them under that metric (fdr_sparse_rescore) and writes the
    best nndescent_n_neighbors with the exact distances.  radius_rescore (with radius, a sparse metric's name): the
    feature rows go to the device once with those values (fdr_rescore_rows_build), and each row block's projected hits
    are scored on them and cut at radius_rescore_bound (None: 1) in that metric (fdr_rescore_rows_radius).  symmetrize
    ("union" / "mutual"; None: the rows as searched): whichever of these modes ran, the graph it is about to write is
    symmetrised on the GPU first (fdr_graph_symmetrize) and written once through fdr_overlaps_write_csr.  components
    ((mode, max_distance); None: no components.tsv): the connected components of the rows as searched, before any
    symmetrize, are found on the GPU (fdr_graph_components) and written to components.tsv beside overlaps.tsv.  refine
    (projected k-NN mode, a sparse metric's name): the lists of the search, re-scored or not, go through refine_rounds
    rounds of RescoreRows.refine on the feature rows held on the device, with refine_fan (None: min(k, FDR_MAX_K))
    and refine_reverse, before they are written (refined_lists)."""
    from . import _lib
    from .feature_extraction import _projection_csr
    if kmer_searcher_output:
        logger.info("--- 1. (skipped) using kmer_searcher output %s ---", kmer_searcher_output)
    else:
        logger.info("--- 1. (skipped) using feature matrix %s ---", feature_matrix)
    indptr, indices, n_features, P, read_names, strands = load_inputs(
        output_dir=output_dir, embedding_dimension=embedding_dimension, save_feature_matrix=save_feature_matrix,
        kmer_searcher_output=kmer_searcher_output, kmer_library=kmer_library, feature_matrix=feature_matrix,
        kmer_counts=kmer_counts, read_names_path=read_names_path, no_projection=no_projection,
        metric=no_projection_metric)
    ctx = _lib.default_context()
    if no_projection and no_projection_radius is not None:
        logger.info("--- 4. Radius search (exact, metric = %s, radius = %g, on the feature rows) ---",
                    no_projection_metric, no_projection_radius)
        logger.info("--no-projection-radius: -n/--embedding-dimension (%d) and --nndescent-n-neighbors (%d) are "
                    "ignored; %d rows x %d features, %d stored entries", embedding_dimension, nndescent_n_neighbors,
                    indptr.size - 1, n_features, indices.size)
        values = None if no_projection_metric == "jaccard" else P[indices]
        with ctx.sparse_index(indptr, indices, values, n_features, metric=no_projection_metric) as index:
            rows = write_radius_overlaps(join(output_dir, "overlaps.tsv"), index, no_projection_radius, read_names,
                                         strands, symmetrize=symmetrize, ctx=ctx, components=components)
        logger.debug("wrote %d overlap rows", rows)
        _cleanup(keep_intermediates)
        return
    if no_projection and no_projection_metric == "jaccard":
        logger.info("--- 4. Nearest Neighbors Search (exact, metric = jaccard, on the feature sets) ---")
        logger.info("--no-projection: -n/--embedding-dimension (%d) is ignored; %d rows x %d features, %d stored "
                    "entries", embedding_dimension, indptr.size - 1, n_features, indices.size)
        neighbor_matrix, distances = ctx.knn_sparse(indptr, indices, None, n_features, nndescent_n_neighbors,
                                                    metric="jaccard")
        _finish(output_dir, neighbor_matrix, distances, read_names, strands, keep_intermediates, symmetrize, ctx, components)
        return
    if no_projection:
        logger.info("--- 4. Nearest Neighbors Search (exact, metric = %s, on the IDF-weighted feature rows) ---",
                    no_projection_metric)
        logger.info("--no-projection: -n/--embedding-dimension (%d) is ignored; %d rows x %d features, %d stored "
                    "entries", embedding_dimension, indptr.size - 1, n_features, indices.size)
        neighbor_matrix, distances = ctx.knn_sparse(indptr, indices, P[indices], n_features, nndescent_n_neighbors,
                                                    metric=no_projection_metric)
        _finish(output_dir, neighbor_matrix, distances, read_names, strands, keep_intermediates, symmetrize, ctx, components)
        return
    Pc = _projection_csr(P)
    ctx.projection_load(Pc.indptr, Pc.indices, Pc.data, n_features, embedding_dimension)
    cip, cix = ctx.csr_compact(indptr, indices)
    logger.debug("embedding %d rows: %d of %d feature ids have an entry in P", indptr.size - 1, cix.size, indices.size)

    def rescore_values(metric):  # the values of --no-projection under this metric
        if metric == "jaccard":
            return None
        from .precompute import read_kmer_counts
        counts = read_kmer_counts(kmer_library) if kmer_searcher_output else _load_counts(kmer_counts)
        return sparse_weights(counts, n_features, metric)[indices]

    if rescore is not None:
        n, k = indptr.size - 1, nndescent_n_neighbors
        kp = default_rescore_candidates(k, n) if rescore_candidates is None else rescore_candidates
        if not k <= kp <= min(_lib.FDR_MAX_K, n):
            raise SystemExit("--rescore needs --nndescent-n-neighbors = %d <= K' = %d <= min(%d, the %d reads)"
                             % (k, kp, _lib.FDR_MAX_K, n))
        logger.info("--- 4. Nearest Neighbors Search (projected, K' = %d), re-scored on the feature rows (metric = %s, "
                    "k = %d) ---", kp, rescore, k)
        candidates, _ = ctx.embed_knn(cip, cix, kp)
        del cip, cix
        values = rescore_values(rescore)
        neighbor_matrix, distances = ctx.sparse_rescore(indptr, indices, values, n_features, candidates, k=k,
                                                        metric=rescore)
        if refine is not None:
            graph = refined_lists(ctx, (indptr, indices, values, n_features), refine, (neighbor_matrix, distances), k,
                                  refine_fan, refine_rounds, refine_reverse)
            _finish_ragged(output_dir, graph, read_names, strands, keep_intermediates, symmetrize, ctx, components)
            return
        _finish(output_dir, neighbor_matrix, distances, read_names, strands, keep_intermediates, symmetrize, ctx, components)
        return
    if radius is not None and radius_rescore is not None:
        bound = 1.0 if radius_rescore_bound is None else radius_rescore_bound
        logger.info("--- 4. Radius search (projected rows, cosine, radius = %g), re-scored on the feature rows (metric = "
                    "%s, bound = %g) ---", radius, radius_rescore, bound)
        logger.info("--radius: --nndescent-n-neighbors (%d) is ignored; %d rows, d = %d", nndescent_n_neighbors,
                    cip.size - 1, embedding_dimension)
        with ctx.dense_index_from_csr(cip, cix) as index, \
                ctx.rescore_rows(indptr, indices, rescore_values(radius_rescore), n_features,
                                 metric=radius_rescore) as held:
            del cip, cix
            both = RescoredRadius(index, held, bound)
            rows = write_radius_overlaps(join(output_dir, "overlaps.tsv"), both, radius, read_names, strands,
                                         symmetrize=symmetrize, ctx=ctx, components=components)
        logger.debug("wrote %d overlap rows of %d projected hits", rows, both.candidates)
        _cleanup(keep_intermediates)
        return
    if refine is not None:
        k = nndescent_n_neighbors
        logger.info("--- 4. Nearest Neighbors Search (projected, k = %d), refined on the feature rows ---", k)
        lists = ctx.embed_knn(cip, cix, k)
        del cip, cix
        graph = refined_lists(ctx, (indptr, indices, rescore_values(refine), n_features), refine, lists, k, refine_fan,
                              refine_rounds, refine_reverse)
        _finish_ragged(output_dir, graph, read_names, strands, keep_intermediates, symmetrize, ctx, components)
        return
    del indptr, indices
    if radius is not None:
        logger.info("--- 4. Radius search (projected rows, cosine, radius = %g) ---", radius)
        logger.info("--radius: --nndescent-n-neighbors (%d) is ignored; %d rows, d = %d", nndescent_n_neighbors,
                    cip.size - 1, embedding_dimension)
        with ctx.dense_index_from_csr(cip, cix) as index:
            rows = write_radius_overlaps(join(output_dir, "overlaps.tsv"), index, radius, read_names, strands,
                                         symmetrize=symmetrize, ctx=ctx, components=components)
        logger.debug("wrote %d overlap rows", rows)
        _cleanup(keep_intermediates)
        return
    logger.info("--- 4. Nearest Neighbors Search ---")
    logger.info("Using exact GPU k-NN in place of NNDescent (n_trees = %s, leaf_size = %s are inert)",
                nndescent_n_trees, 200)
    neighbor_matrix, distances = ctx.embed_knn(cip, cix, nndescent_n_neighbors)
    _finish(output_dir, neighbor_matrix, distances, read_names, strands, keep_intermediates, symmetrize, ctx, components)


def _finish(output_dir, neighbor_matrix, distances, read_names, strands, keep_intermediates, symmetrize=None, ctx=None,
            components=None):
    nbr_output_file = join(output_dir, "overlaps.tsv")
    logger.debug("Saving overlap table to %s", nbr_output_file)
    if symmetrize is not None or components is not None:
        graph = (np.ascontiguousarray(neighbor_matrix, dtype=np.int32), np.ascontiguousarray(distances, dtype=np.float32))
    if components is not None:
        write_components(join(output_dir, "components.tsv"), ctx, graph, components[0], components[1], read_names,
                         strands)
    if symmetrize is not None:
        rows = write_symmetrized(nbr_output_file, ctx, graph, symmetrize, read_names, strands)
    else:
        rows = write_overlaps(nbr_output_file, neighbor_matrix, distances, read_names, strands)
    logger.debug("wrote %d overlap rows", rows)
    _cleanup(keep_intermediates)


def refined_lists(ctx, rows, metric, graph, k, fan=None, rounds=1, reverse=False):
    """--refine: `rounds` rounds of RescoreRows.refine at k on the feature rows `rows` = (indptr, indices, values,
    n_features) under `metric`, held on the device for all of them; round 1 starts from `graph` (the search's lists),
    round i from round i - 1's rows.  Returns the last round's ragged (indptr, idx, dist)."""
    indptr, indices, values, n_features = rows
    with ctx.rescore_rows(indptr, indices, values, n_features, metric=metric) as held:
        for i in range(rounds):
            graph = held.refine(graph, k, fan=fan, reverse=reverse)
            logger.info("--refine %s: round %d of %d left %d entries of %d rows", metric, i + 1, rounds,
                        int(graph[0][-1]), graph[0].size - 1)
    ctx.graph_free()
    return graph


def _finish_ragged(output_dir, graph, read_names, strands, keep_intermediates, symmetrize=None, ctx=None,
                   components=None):
    """_finish for a ragged (indptr, idx, dist), every row ascending by (distance bits, index): through
    fdr_overlaps_write_csr."""
    from . import _lib
    nbr_output_file = join(output_dir, "overlaps.tsv")
    logger.debug("Saving overlap table to %s", nbr_output_file)
    if components is not None:
        write_components(join(output_dir, "components.tsv"), ctx, graph, components[0], components[1], read_names,
                         strands)
    if symmetrize is not None:
        rows = write_symmetrized(nbr_output_file, ctx, graph, symmetrize, read_names, strands)
    else:
        name_off, names = _lib.pack_names(read_names)
        rows = _lib.overlaps_write_csr(nbr_output_file, *graph, name_off, names, np.asarray(strands, dtype=np.uint8),
                                       n_threads=global_variables.threads if global_variables.threads > 1 else 0)
    logger.debug("wrote %d overlap rows", rows)
    _cleanup(keep_intermediates)


def _cleanup(keep_intermediates):
    if not keep_intermediates and global_variables.temp_dir and os.path.isdir(global_variables.temp_dir):
        logger.debug("Removing intermediate files")
        rmtree(global_variables.temp_dir)
    logger.info("Pipeline completed.")


def record_names(name_off, name_buf):
    """(name_off, names) of the R records as fdr_overlaps_write takes them in its doubled-rows mode (strands=None: row
    t carries record t >> 1's id -- no id is materialised twice, let alone gathered byte by byte).  Valid UTF-8 ids
    pass through untouched; ids that are not follow the reference's rule (feature_extraction.py:125-128) through the
    str path."""
    from . import _lib
    from .feature_extraction import _decode_names
    raw = name_buf.tobytes()
    if not raw.isascii():
        try:
            raw.decode("utf-8")
        except UnicodeDecodeError:
            return _lib.pack_names(_decode_names(name_off, name_buf))
    return name_off, name_buf


def load_rank_inputs(args, output_dir, rank, world):
    """What ONE rank of `--devices` needs on the host: the projection matrix, ITS row block of the read x feature
    CSR (1 / world of the matrix: the ranged native loader for output.bin; a feature_matrix.npz is inflated whole
    and sliced, scipy's format has no random access) and the names / strands of all rows for the writer.
    Returns (n_rows, lo, hi, indptr, indices, n_features, P, name_off, names, strands); strands is None when
    name_off / names describe the R records of a doubled matrix (fdr_overlaps_write's doubled-rows mode).  With
    --no-projection the feature weights take P's place (sparse_weights, as in load_inputs: None for jaccard)."""
    from . import _lib
    from .distributed import local_csr, shard_rows
    if args.kmer_searcher_output:
        from .precompute import read_kmer_counts
        n_features = 2 * int(read_kmer_counts(args.kmer_library).size)  # (count_kmers.py:148)
        if args.no_projection:
            P = sparse_weights(read_kmer_counts(args.kmer_library), n_features, args.no_projection_metric)
        else:
            P, n_features = get_precompute_matrix(n_components=args.embedding_dimension,
                                                  counter_file=args.kmer_library, n_features=n_features)
        try:
            R = _lib.kmer_output_records(args.kmer_searcher_output)  # (the header's count: no record is walked for it)
            n = 2 * R
            _, blocks = shard_rows(n, world)
            lo, hi = blocks[rank]
            _, ip, ix, name_off, name_buf = _lib.kmer_output_load_range(
                args.kmer_searcher_output, n_features, lo // 2, hi // 2,
                n_threads=global_variables.threads if global_variables.threads > 1 else 0)
        except _lib.FedrannHipError as e:
            if "output.bin:" in str(e):  # format errors keep the reference's exception type
                raise ValueError(str(e).split("output.bin:", 1)[1].strip()) from None
            raise
        name_off, names = record_names(name_off, name_buf)
        strands = None  # (fdr_overlaps_write's doubled-rows mode: row t = record t >> 1 on strand t & 1)
        if args.save_feature_matrix and rank == 0:  # (the whole matrix, once)
            from .feature_extraction import build_feature_csr
            fip, fix, _, _ = build_feature_csr(args.kmer_searcher_output, n_features)
            save_feature_matrix_npz(join(output_dir, "feature_matrix.npz"), fip, fix, n_features)
            del fip, fix
    else:
        indptr, indices, n_features = load_feature_matrix_npz(args.feature_matrix)
        if args.no_projection:
            P = sparse_weights(_load_counts(args.kmer_counts), n_features, args.no_projection_metric)
        else:
            P = build_precompute_matrix(_load_counts(args.kmer_counts), args.embedding_dimension,
                                        n_features=n_features)
        n = indptr.size - 1
        _, blocks = shard_rows(n, world)
        lo, hi = blocks[rank]
        if args.save_feature_matrix and rank == 0:
            save_feature_matrix_npz(join(output_dir, "feature_matrix.npz"), indptr, indices, n_features)
        ip, ix = local_csr(indptr, indices, lo, hi)
        del indptr, indices
        read_names, strand_list = _load_names(args.read_names, n)
        name_off, names = _lib.pack_names(read_names)
        strands = np.asarray(strand_list, dtype=np.uint8)
    return n, lo, hi, ip, ix, n_features, P, name_off, names, strands


def run_rank_worker(args, output_dir, temp_dir):
    """One rank of `--devices`: RANK / WORLD_SIZE / FEDRANN_DEVICE / FEDRANN_RENDEZVOUS come from the parent, and
    so do the byte-range cuts of the reads (--stage1-cuts) when the run starts from reads: the rank then runs its
    share of stage 1 (stage1_sharded.run_stage1_rank), which leaves temp/kmer_searcher/output.bin and the library
    for all ranks.  A rank loads ITS rows of the feature matrix, embeds them, the normalised blocks are all-gathered,
    it searches its rows against all rows (distributed.ShardedPipeline) and writes temp/overlaps.rank<r>.tsv."""
    import datetime
    import torch
    import torch.distributed as dist
    from . import _lib
    from .distributed import HipEngine, ShardedPipeline
    from .feature_extraction import _projection_csr
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    device = torch.device("cuda", int(os.environ["FEDRANN_DEVICE"]))
    torch.cuda.set_device(device)
    # rendezvous through a file in temp/ (no port to lose to another process); the host stages between two
    # collectives (loading a rank's rows of a 10 M-read matrix, writing its part of overlaps.tsv) may take long
    # (FEDRANN_COLLECTIVE_TIMEOUT_S: how long a rank waits inside one collective, default 2 h -- the long host stages
    # between two collectives are a rank's share of stage 1, bounded by its byte range, and the load below, and a
    # barrier right after each takes that wait; a rank that hangs without dying no longer holds its siblings for half a
    # day)
    kw = dict(init_method="file://" + os.environ["FEDRANN_RENDEZVOUS"], rank=rank, world_size=world,
              timeout=datetime.timedelta(seconds=float(os.environ.get("FEDRANN_COLLECTIVE_TIMEOUT_S", "7200"))))
    if args.dist_backend == "nccl":
        dist.init_process_group("nccl", device_id=device, **kw)
    else:
        dist.init_process_group("gloo", **kw)
    ctx = _lib.Context(device.index)
    if args.stage1_cuts:
        from .stage1_sharded import parse_cuts, run_stage1_rank
        is_fastq, cuts = parse_cuts(args.stage1_cuts)
        if rank == 0:
            logger.info("--- 1. k-mer %s over %d GPUs ---", "search" if args.kmer_library else "counting and search",
                        world)
        args.kmer_searcher_output, args.kmer_library = run_stage1_rank(args, temp_dir, ctx, device, args.dist_backend,
                                                                       cuts, is_fastq, args.input)
    k = args.nndescent_n_neighbors
    if args.no_projection and args.no_projection_radius is not None:
        lo, hi, rows = _sparse_rank_radius(args, output_dir, ctx, rank, world,
                                           join(temp_dir, "overlaps.rank%d.tsv" % rank))
        logger.debug("rank %d: rows [%d, %d), %d overlap rows", rank, lo, hi, rows)
        dist.barrier()
        dist.destroy_process_group()
        ctx.close()
        return
    if args.no_projection:
        idx, dst, lo, name_off, names, strands = _sparse_rank_search(args, output_dir, ctx, rank, world, k)
        part = join(temp_dir, "overlaps.rank%d.tsv" % rank)
        rows = _lib.overlaps_write(part, idx, dst, name_off, names, strands, row0=lo, header=rank == 0,
                                   n_threads=global_variables.threads if global_variables.threads > 1 else 0)
        logger.debug("rank %d: rows [%d, %d), %d overlap rows", rank, lo, lo + idx.shape[0], rows)
        dist.barrier()
        dist.destroy_process_group()
        ctx.close()
        return
    n, lo, hi, ip, ix, n_features, P, name_off, names, strands = load_rank_inputs(args, output_dir, rank, world)
    dist.barrier()  # every rank has its rows: what follows is GPU work and short collectives
    Pc = _projection_csr(P)
    ctx.projection_load(Pc.indptr, Pc.indices, Pc.data, n_features, args.embedding_dimension)
    pipe = ShardedPipeline(HipEngine(ctx, device), n, args.embedding_dimension, k, rank=rank, world_size=world,
                           device=device)
    assert (pipe.lo, pipe.hi) == (lo, hi)
    logger.debug("rank %d of %d holds rows [%d, %d) of %d: %d column ids", rank, world, lo, hi, n, ix.size)
    ip, ix = ctx.csr_compact(ip, ix)
    if rank == 0:
        logger.info("--- 4. Nearest Neighbors Search (%d rows over %d GPUs) ---", n, world)
    idx, dst, _ = pipe.step(torch.from_numpy(ip).to(device), torch.from_numpy(ix).to(device))
    torch.cuda.synchronize(device)
    part = join(temp_dir, "overlaps.rank%d.tsv" % rank)
    rows = _lib.overlaps_write(part, idx.cpu().numpy(), dst.cpu().numpy(), name_off, names, strands, row0=lo,
                               header=rank == 0,
                               n_threads=global_variables.threads if global_variables.threads > 1 else 0)
    logger.debug("rank %d: rows [%d, %d), %d overlap rows", rank, lo, hi, rows)
    dist.barrier()
    dist.destroy_process_group()
    ctx.close()


def _sparse_rank_search(args, output_dir, ctx, rank, world, k):
    """Stage 4 of one rank of `--no-projection --devices ... --sparse-shard ...`: (idx, dist, lo, name_off, names,
    strands), the rank's rows [lo, lo + rows) of the one-GPU search and what the writer needs.
    targets: the rank loads ITS row block (load_rank_inputs) and runs distributed.sparse_knn_sharded, whose collectives
    travel on a gloo group.  queries: the rank loads the whole matrix (load_inputs) and runs distributed.sparse_knn_rank;
    no collective beyond the worker's barriers."""
    import torch.distributed as dist
    from . import _lib
    from .distributed import sparse_knn_rank, sparse_knn_sharded
    metric = args.no_projection_metric
    if args.sparse_shard == "targets":
        n, lo, hi, ip, ix, n_features, w, name_off, names, strands = load_rank_inputs(args, output_dir, rank, world)
        dist.barrier()  # every rank has its rows
        if rank == 0:
            logger.info("--- 4. Nearest Neighbors Search (exact, metric = %s, %d rows, targets over %d GPUs) ---",
                        metric, n, world)
        logger.debug("rank %d of %d holds rows [%d, %d) of %d: %d column ids", rank, world, lo, hi, n, ix.size)
        try:
            got = sparse_knn_sharded(ctx, ip, ix, None if w is None else w[ix], n_features, k, metric=metric,
                                     block_rows=SPARSE_QUERY_BLOCK_ROWS)
        except ValueError as e:  # (k above a rank's rows: the same words on every rank, before any GPU work)
            raise SystemExit("--sparse-shard targets: %s" % e) from None
        assert got[:2] == (lo, hi)
        return got[2], got[3], lo, name_off, names, strands
    indptr, indices, n_features, w, read_names, strand_list = load_inputs(
        output_dir=output_dir, embedding_dimension=args.embedding_dimension,
        save_feature_matrix=args.save_feature_matrix, kmer_searcher_output=args.kmer_searcher_output,
        kmer_library=args.kmer_library, feature_matrix=args.feature_matrix, kmer_counts=args.kmer_counts,
        read_names_path=args.read_names, save=rank == 0, no_projection=True, metric=metric)
    dist.barrier()  # every rank has the matrix
    if rank == 0:
        logger.info("--- 4. Nearest Neighbors Search (exact, metric = %s, %d rows, queries over %d GPUs) ---", metric,
                    indptr.size - 1, world)
    lo, hi, idx, dst = sparse_knn_rank(ctx, indptr, indices, None if w is None else w[indices], n_features, k, rank,
                                       world, metric=metric, block_rows=SPARSE_QUERY_BLOCK_ROWS)
    name_off, names = _lib.pack_names(read_names)
    return idx, dst, lo, name_off, names, np.asarray(strand_list, dtype=np.uint8)


def _sparse_rank_radius(args, output_dir, ctx, rank, world, part):
    """Stage 4 of one rank of `--no-projection --no-projection-radius R --devices ... --sparse-shard targets`: the rank
    loads ITS row block (load_rank_inputs), runs distributed.sparse_radius_sharded (collectives on a gloo group) and
    writes its rows [lo, hi) of the one-GPU radius search to `part` through fdr_overlaps_write_csr, the header on rank 0
    only.  RADIUS_BLOCK_ROWS / RADIUS_MAX_HITS bound a device call as on one GPU.  Returns (lo, hi, data lines)."""
    import torch.distributed as dist
    from . import _lib
    from .distributed import sparse_radius_sharded
    metric = args.no_projection_metric
    n, lo, hi, ip, ix, n_features, w, name_off, names, strands = load_rank_inputs(args, output_dir, rank, world)
    dist.barrier()  # every rank has its rows
    if rank == 0:
        logger.info("--- 4. Radius search (exact, metric = %s, radius = %g, %d rows, targets over %d GPUs) ---", metric,
                    args.no_projection_radius, n, world)
    logger.debug("rank %d of %d holds rows [%d, %d) of %d: %d column ids", rank, world, lo, hi, n, ix.size)
    try:
        got = sparse_radius_sharded(ctx, ip, ix, None if w is None else w[ix], n_features, args.no_projection_radius,
                                    metric=metric, block_rows=RADIUS_BLOCK_ROWS, max_hits=RADIUS_MAX_HITS)
    except ValueError as e:  # (a rank without rows, a row above the cap: before the file is begun)
        raise SystemExit("--sparse-shard targets: %s" % e) from None
    assert got[:2] == (lo, hi)
    rows = _lib.overlaps_write_csr(part, got[2], got[3], got[4], name_off, names, strands, row0=lo, header=rank == 0,
                                   n_threads=global_variables.threads if global_variables.threads > 1 else 0)
    return lo, hi, rows


def launch_rank_workers(argv, args, devices, output_dir, temp_dir, keep_intermediates):
    """The parent of `--devices`: no GPU call here (a process that has initialised the GPU must not start
    others on this pool, and the children own the devices).  Children = this module with --rank-worker (one per
    device).  From reads, the parent decompresses a .gz input into temp/ and cuts the plain file into one byte range
    per rank (stage1_sharded.cut_ranges, a few KiB read around each cut); the ranks run stage 1 between them."""
    import time
    argv = list(argv)
    if args.input and not args.kmer_searcher_output and not args.feature_matrix:
        from .stage1_sharded import cut_ranges, format_cuts
        reads = args.input
        if reads.endswith(".gz"):
            import gzip
            plain = join(temp_dir, os.path.basename(reads[:-3]))
            with gzip.open(reads, "rb") as src, open(plain, "wb") as dst:
                copyfileobj(src, dst, 1 << 24)
            reads = plain
        if not args.kmer_library and not reads.endswith((".fasta", ".fa", ".fastq", ".fq")):
            raise ValueError("Unsupported file format. Please provide a FASTA or FASTQ file.")  # (as run_kmer_searcher)
        is_fastq, cuts = cut_ranges(reads, len(devices))
        logger.debug("stage 1 byte ranges: %s", cuts)
        argv += ["-i", abspath(reads), "--stage1-cuts", format_cuts(is_fastq, cuts)]
    rendezvous = join(temp_dir, "rendezvous.%d" % os.getpid())
    if os.path.exists(rendezvous):
        os.remove(rendezvous)
    procs = []
    for rank, dev in enumerate(devices):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(len(devices)), LOCAL_RANK=str(rank),
                   FEDRANN_DEVICE=str(dev), FEDRANN_RENDEZVOUS=rendezvous)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (RCCL between processes needs dmabuf IPC on hosts like this pool's)
        procs.append(subprocess.Popen([sys.executable, "-m", "fedrann_amd"] + argv + ["--rank-worker"], env=env))
    # poll all ranks: the first failure ends the others (they would sit in a collective until its timeout); whatever ends
    # the parent -- KeyboardInterrupt, SIGTERM turned into SystemExit, an error here -- ends the ranks and removes the
    # rendezvous file too
    codes = [None] * len(procs)

    def end_ranks():
        for i, p in enumerate(procs):
            if codes[i] is None and p.poll() is None:
                p.terminate()
        for i, p in enumerate(procs):
            if codes[i] is None:
                try:
                    codes[i] = p.wait(timeout=10)
                except subprocess.TimeoutExpired:
                    p.kill()
                    codes[i] = p.wait()

    import signal
    old_term = signal.signal(signal.SIGTERM, lambda *_: sys.exit(143))
    try:
        while any(c is None for c in codes):
            for i, p in enumerate(procs):
                if codes[i] is None:
                    codes[i] = p.poll()
            if any(c not in (None, 0) for c in codes):
                end_ranks()
                break
            time.sleep(0.05)
    finally:
        end_ranks()
        signal.signal(signal.SIGTERM, old_term)
        if os.path.exists(rendezvous):
            os.remove(rendezvous)
    if any(codes):
        raise SystemExit("rank worker(s) failed: exit codes %s" % codes)
    out = join(output_dir, "overlaps.tsv")
    with open(out, "wb") as dst:
        for rank in range(len(devices)):
            with open(join(temp_dir, "overlaps.rank%d.tsv" % rank), "rb") as src:
                copyfileobj(src, dst, 1 << 24)
    if not keep_intermediates and os.path.isdir(temp_dir):
        rmtree(temp_dir)
    logger.info("Pipeline completed.")


def _gpu_kmer_search(reads_path, fwd_library, k, temp_dir):
    """reads + forward library -> temp/kmer_searcher/output.bin (and kmer_frequency.bin).  The reverse
    library is the reverse complement of every forward k-mer, in the same order (`seqkit seq -r -p`,
    count_kmers.py:127); both are passed in the reference's order: forward, then reverse."""
    from .kmer_search import kmer_searcher
    from .stage1_sharded import reverse_library_text
    with open(fwd_library, "rb") as f:
        rev_text = reverse_library_text(f.read())
    rev_path = join(temp_dir, "rev_kmer_library.fasta")
    with open(rev_path, "wb") as f:
        f.write(rev_text)
    if reads_path.endswith(".gz"):
        import gzip
        plain = join(temp_dir, os.path.basename(reads_path[:-3]))
        with gzip.open(reads_path, "rb") as src, open(plain, "wb") as dst:
            copyfileobj(src, dst, 1 << 24)
        reads_path = plain
    out_dir = join(temp_dir, "kmer_searcher")
    n_reads, _, nnz, n_lib = kmer_searcher([fwd_library, rev_path], reads_path, out_dir, k, fastq_ids_as_fasta=True,
                                           collect=False)  # (the reference runs seqkit fq2fa first; reads streamed)
    logger.debug("k-mer search: %d reads, %d library k-mers, %d hits", n_reads, n_lib, nnz)
    return join(out_dir, "output.bin")


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse_command_line_arguments(argv)
    global_variables.threads = args.threads
    global_variables.seed = args.seed
    check_limits(1 if args.no_projection else args.embedding_dimension,  # (-n is not used without the projection)
                 # (... nor --nndescent-n-neighbors by a radius search)
                 1 if args.no_projection_radius is not None or args.radius is not None else args.nndescent_n_neighbors)
    # (before any work: the library would only refuse them after stages 1-3)
    check_radius(args, "--no-projection-radius", args.no_projection_radius, True)
    check_radius(args, "--radius", args.radius, False)
    check_sparse_shard(args)
    check_rescore(args)
    check_symmetrize(args)
    check_components(args)
    radius_rescore_bound = check_radius_rescore(args)
    refine_fan, refine_rounds = check_refine(args)
    if args.no_projection_metric != "cosine" and not args.no_projection:
        raise SystemExit("--no-projection-metric %s needs --no-projection (the projected search is cosine only)"
                         % args.no_projection_metric)
    if args.device is not None and not args.rank_worker:
        os.environ["FEDRANN_DEVICE"] = str(args.device)
    output_dir = abspath(args.output_dir)
    os.makedirs(output_dir, exist_ok=True)
    global_variables.output_dir = output_dir
    _setup_logging(join(output_dir, "fedrann.log"))
    temp_dir = join(output_dir, "temp")
    os.makedirs(temp_dir, exist_ok=True)
    global_variables.temp_dir = temp_dir
    have_ks = bool(args.kmer_searcher_output)
    have_fm = bool(args.feature_matrix)
    if sum((bool(args.input), have_ks, have_fm)) != 1:
        raise SystemExit(
            "give exactly one of -i reads, -i reads + --kmer-library, --kmer-searcher-output + --kmer-library, "
            "or --feature-matrix + --kmer-counts")
    if have_ks and not args.kmer_library:
        raise SystemExit("--kmer-searcher-output needs --kmer-library")
    if have_fm and not args.kmer_counts:
        raise SystemExit("--feature-matrix needs --kmer-counts")
    if args.rank_worker:
        return run_rank_worker(args, output_dir, temp_dir)
    logger.info("FEDRANN (MI355X hot path) version: %s", __version__)
    logger.debug("Parameters: %s", args)
    if args.devices:
        devices = device_list(args.devices)
        if len(devices) > 1:
            return launch_rank_workers(argv, args, devices, output_dir, temp_dir, args.keep_intermediates)
        if devices:
            os.environ["FEDRANN_DEVICE"] = str(devices[0])
    if args.input and args.kmer_library and not have_ks and not have_fm:
        # stage 1b on the GPU: reads x sampled k-mer library -> output.bin (count_kmers.py:119-139 with the
        # reverse library made here instead of by seqkit, the search by fdr_kmer_search instead of kmer_searcher)
        logger.info("--- 1b. k-mer search on the GPU ---")
        args.kmer_searcher_output = _gpu_kmer_search(args.input, args.kmer_library, args.kmer_size, temp_dir)
        have_ks = True
    if args.input and not args.kmer_library and not have_ks and not have_fm:
        # the whole stage 1 on the GPU (count_kmers.py:52-148): canonical k-mer counts, threshold, Bernoulli
        # sample, reverse library, search
        from .count_kmers import run_kmer_searcher
        logger.info("--- 1. Counter kmers (GPU) ---")
        args.kmer_searcher_output, n_features, read_count = run_kmer_searcher(
            input_path=args.input, k=args.kmer_size, sample_fraction=args.kmer_sample_fraction,
            min_multiplicity=args.kmer_min_multiplicity)
        logger.debug("kmer_searcher n_features: %d, reads: %d", n_features, read_count)
        args.kmer_library = join(temp_dir, "fwd_kmer_library.fasta")
        have_ks = True
    run_fedrann_pipeline(
        output_dir=output_dir, embedding_dimension=args.embedding_dimension,
        nndescent_n_trees=args.nndescent_n_trees, nndescent_n_neighbors=args.nndescent_n_neighbors,
        save_feature_matrix=args.save_feature_matrix, keep_intermediates=args.keep_intermediates,
        chunk_size=args.chunk_size, kmer_searcher_output=args.kmer_searcher_output,
        kmer_library=args.kmer_library, feature_matrix=args.feature_matrix,
        kmer_counts=args.kmer_counts, read_names_path=args.read_names, no_projection=args.no_projection,
        no_projection_metric=args.no_projection_metric, no_projection_radius=args.no_projection_radius,
        radius=args.radius, rescore=args.rescore, rescore_candidates=args.rescore_candidates,
        radius_rescore=args.radius_rescore, radius_rescore_bound=radius_rescore_bound, symmetrize=args.symmetrize,
        components=None if args.components is None else (args.components, args.components_distance),
        refine=args.refine, refine_fan=refine_fan, refine_rounds=refine_rounds, refine_reverse=args.refine_reverse)


if __name__ == "__main__":
    main()
