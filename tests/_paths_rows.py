"""Inputs shared by the prefilter-path tests (tests/test_gpu_paths.py) and the candidate-pass tests
(tests/test_gpu_candidates.py): rows that take every way through the prefilter mode, and the table of candidate-pass
kernel variants with the size at which the planner picks each."""
import numpy as np

RESERVED = 4  # trailing dimensions only the "lonely" rows use


def _plateau_rows(rng, d, clusters, size):
    """`clusters` centres q = 3 e_u + b e_v (b in 2, 4, 5: no two centres proportional), each with `size` members
    q +- e_j (j outside {u, v}).  Integer components: every squared norm is exact, and q . (q +- e_j) = |q|^2 with a zero
    term at j, so all members sit at the same fp32 distance from q and from each other -- distinct rows on exact
    plateaus (duplicates or scaled copies would fall into one duplicate-row class instead)."""
    free = d - RESERVED
    seen, rows = set(), []
    while len(seen) < clusters:
        u, v = rng.choice(free, 2, replace=False)
        b = int(rng.choice((2, 4, 5)))
        su, sv = rng.choice((-1, 1), 2)
        key = (int(u), int(v), b, int(su), int(sv))
        if key in seen:
            continue
        seen.add(key)
        q = np.zeros(d, dtype=np.float32)
        q[u], q[v] = 3 * su, b * sv
        rows.append(q)
        opts = np.array([(j, s) for j in range(free) if j != u and j != v for s in (-1, 1)])
        for j, s in opts[rng.choice(len(opts), size, replace=False)]:
            t = q.copy()
            t[j] = s
            rows.append(t)
    return np.stack(rows)


def _paths_input(n, d, seed, plateau, overflow, zero=8):
    """n distinct rows (but `zero` all-zero ones), shuffled, on the device:
      plateau   (clusters, members): exact-tie plateaus of fewer than RANGE_CAP = 1024 rows -> the range pass
      overflow  clusters of 1100 near-ties (a centre + 1e-4 noise) -> the range pass collects more than RANGE_CAP ->
                FDR_PATH_RANGE_OVERFLOW, the exact kernel
      RESERVED  lonely rows e_j on the reserved dimensions: no target but themselves at a distance below 1 -> the
                certificate fails with d(k) = 1 -> FDR_PATH_EXACT
      the rest  low-rank (24) Gaussian rows: well separated k-th / K'-th neighbours -> certified."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(seed)
    free = d - RESERVED
    parts = [_plateau_rows(rng, d, *plateau)] if plateau[0] else []
    for _ in range(overflow):
        c = rng.standard_normal(free).astype(np.float32)
        blk = np.zeros((1100, d), dtype=np.float32)
        blk[:, :free] = c + np.float32(1e-4) * rng.standard_normal((1100, free)).astype(np.float32)
        parts.append(blk)
    lonely = np.zeros((RESERVED, d), dtype=np.float32)
    lonely[np.arange(RESERVED), free + np.arange(RESERVED)] = 1.0
    parts += [lonely, np.zeros((zero, d), dtype=np.float32)]
    S = torch.from_numpy(np.concatenate(parts)).to(dev)
    nb = n - S.shape[0]
    assert nb > n // 4, (n, S.shape)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    B = torch.randn((24, free), device=dev, generator=g)
    E = torch.zeros((n, d), dtype=torch.float32, device=dev)
    E[:nb, :free] = torch.randn((nb, 24), device=dev, generator=g) @ B
    E[nb:] = S
    return E[torch.randperm(n, device=dev, generator=g)].contiguous()


def _normalize(ctx, E):
    import torch
    n, d = E.shape
    dp = ctx.padded_dim(d)
    Ehat = torch.zeros((n, dp), dtype=torch.float32, device=E.device)
    zero = torch.zeros((n,), dtype=torch.uint8, device=E.device)
    ctx.normalize_dev(E.data_ptr(), n, d, Ehat.data_ptr(), zero.data_ptr())
    return Ehat, zero


# (name, d, k, size as a multiple of 512 * CUs query rows, input mix, the candidate pass's shape, one launch?, fallback)
#   input mix: "mixed" = 12 plateaus of 200 (one range chunk < 4096: the four-wave range kernel) + one overflow cluster;
#   "heavy" = 80 plateaus + 17 overflow clusters (34.8 k plateau queries: a ping-pong range chunk of 32 768, then a
#   four-wave one of ~2 k; 18.7 k uncertified rows: the exact kernel in two chunks); "whole" = overflow clusters for
#   more than half the rows (several ping-pong range chunks, then the exact kernel for the whole call)
MIX = {"mixed": ((12, 200), 1), "heavy": ((80, 200), 17)}
CASES = [
    # DP 128: four-wave (168 ... 128 VGPRs, two-unit stages) in one launch; the eight-wave four-unit shape (W8U4) from
    # 1.8 query blocks of 256 per CU, in one launch and in rounds; K' = 62 (2 x 32-key lists): four-wave in rounds
    ("d128_four_wave_one_launch", 128, 20, 0.45, "heavy", (4, 4, 4, 16, 0), True, "chunked"),
    ("d128_w8u4_one_launch", 128, 20, 0.95, "mixed", (8, 4, 8, 16, 0), True, "chunked"),
    ("d128_w8u4_rounds", 128, 20, 1.15, "whole", (8, 4, 8, 16, 0), False, "whole"),
    ("d128_four_wave_32key_rounds", 128, 50, 1.15, "heavy", (4, 4, 4, 32, 0), False, "chunked"),
    # DP 256: below 512 query blocks of 256 per CU the 168-VGPR (K' <= 32) / 256-VGPR four-unit (K' > 32) shapes, from
    # there the ping-pong kernel <256, 8, 16> / <256, 8, 32>
    ("d256_168vgpr", 256, 20, 0.75, "heavy", (4, 3, 4, 16, 0), True, "chunked"),
    ("d256_256vgpr_four_unit", 256, 50, 0.75, "whole", (4, 2, 8, 32, 0), False, "whole"),
    ("d256_pingpong_16", 256, 20, 1.15, "mixed", (8, 2, 16, 16, 1), False, "chunked"),
    ("d256_pingpong_32", 256, 50, 1.15, "heavy", (8, 2, 16, 32, 1), False, "chunked"),
    # DP 512 (d = 500): four-wave four-unit x16 / x32, then ping-pong <512, 8, 16> (eight-unit) / <512, 4, 32> (four-unit)
    ("d500_four_wave_four_unit_16", 500, 20, 0.75, "whole", (4, 2, 8, 16, 0), False, "whole"),
    ("d500_four_wave_four_unit_32", 500, 50, 0.75, "heavy", (4, 2, 8, 32, 0), False, "chunked"),
    ("d500_pingpong_16", 500, 20, 1.15, "mixed", (8, 2, 16, 16, 1), False, "chunked"),
    ("d500_pingpong_32", 500, 50, 1.15, "heavy", (8, 2, 8, 32, 1), False, "chunked"),
]
