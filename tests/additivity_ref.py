"""The additivity measure of the gradient reductions ("Additivity").

Every gradient the library returns is an fp32 sum of per-block partial records (rows). A call on
one row's rays alone returns that row's partial bit for bit (every add is 0 + v), so the terms of
the sum are observable, and the sum has a reference that needs no tolerance: with G the full
call's gradient, G_row the one-row calls' and n non-zero rows,

    |G - sum_rows G_row (in fp64)| <= gamma_(n-1) * A,   A = sum_rows |G_row|,
    gamma_k = k u / (1 - k u), u = 2^-24,

elementwise -- the bound of any fp32 summation tree over n terms (adds of exact zeros are exact,
so n counts the non-zero rows only; n = 1 is bit equality). A row lost, doubled, stale or read at
another column breaks it by the size of a row.

Also here: the kernels' own summation orders restated in numpy from the comments of
csrc/rm_reduce.h (pass 1, pass 2) and csrc/rm_small.h (small_final's chains), for the CPU test of
the measure, and the packing of a gradient dict into one vector.
"""
import numpy as np

U = 2.0 ** -24
K_REDUCE_SEGS = 128            # rm_kernels.hip kReduceSegs
K_SMALL_FINAL_MAX_BLOCKS = 128  # rm_small.h kSmallFinalMaxBlocks
KEYS = ("centers", "colors", "radius", "light_dir", "ambient")


def gamma(k):
    """gamma_k = k u / (1 - k u) (0 for k <= 0)."""
    k = max(int(k), 0)
    return k * U / (1.0 - k * U)


def measure(G, rows, A=None, n=None, factor=1.0):
    """Elementwise additivity of G (E,) against its terms rows (R, E).

    A: the elementwise sum of the terms' magnitudes (default: from `rows`); n: the number of
    non-zero rows of the full call (default: the rows of `rows` with any non-zero element);
    factor: 2 where the terms carry sums of their own (the oracle-A rule).
    Returns (ok, worst err / bound over the elements with a positive bound, n). An element whose
    bound is 0 must be reproduced exactly."""
    G = np.asarray(G, np.float64).reshape(-1)
    rows = np.asarray(rows, np.float64).reshape(-1, G.size)
    if n is None:
        n = int(np.count_nonzero(np.any(rows != 0.0, axis=1)))
    ref = rows.sum(axis=0)
    A = np.abs(rows).sum(axis=0) if A is None else np.asarray(A, np.float64).reshape(-1)
    bound = factor * gamma(n - 1) * A
    err = np.abs(G - ref)
    ok = bool(np.isfinite(G).all() and (err <= bound).all())
    pos = bound > 0.0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    if (err[~pos] > 0.0).any():
        ratio = float("inf")
    return ok, ratio, n


# ---- the kernels' orders, restated ------------------------------------------------------------

def chain(rows, ncols):
    """One fp32 addition chain per column over `rows` (k, ncols) in order, from 0."""
    acc = np.zeros(ncols, np.float32)
    for r in rows:
        acc = acc + np.asarray(r, np.float32)
    return acc


def reduce_segs(nblocks):
    """rm_reduce.h reduce_segs: kReduceSegs segments, or as many multiples of 64 as a launch of
    more than kReduceSegs * 256 blocks needs."""
    need = (nblocks + 255) // 256
    return K_REDUCE_SEGS if need <= K_REDUCE_SEGS else (need + 63) // 64 * 64


def seg_layout(nblocks):
    """(segments, seg_len) of a launch's reduction (reduce_and_finalize)."""
    segs = reduce_segs(nblocks)
    return segs, (nblocks + segs - 1) // segs


def general_order(P, live=None):
    """rm_reduce_partials + finalize of the partial rows P (nb, ncols): pass 1 sums each segment's
    live rows in ray-block order, one chain per column; pass 2 sums the segments in the four chains
    s mod 4, in order, combined (a0 + a1) + (a2 + a3)."""
    P = np.asarray(P, np.float32)
    nb, ncols = P.shape
    live = np.ones(nb, bool) if live is None else np.asarray(live, bool)
    segs, seg_len = seg_layout(nb)
    S = np.zeros((segs, ncols), np.float32)
    for s in range(segs):
        b0, b1 = s * seg_len, min((s + 1) * seg_len, nb)
        S[s] = chain([P[b] for b in range(b0, b1) if live[b]], ncols)
    a = [chain(S[k::4], ncols) for k in range(4)]
    return (a[0] + a[1]) + (a[2] + a[3])


def small_chains(m):
    """small_final's chains per column at m spheres: max(1, min(8, 256 / (8 m + 8)))."""
    return max(1, min(8, 256 // (8 * m + 8)))


def small_order(P, m):
    """rm_small.h small_final on the rows P (nb, ncols): each column by `chains` interleaved chains
    (rows b = ch mod chains, in order), the chains then added in order."""
    P = np.asarray(P, np.float32)
    ncols = P.shape[1]
    c = small_chains(m)
    parts = [chain(P[ch::c], ncols) for ch in range(c)]
    tot = parts[0]
    for p in parts[1:]:
        tot = tot + p
    return tot


# ---- gradient dicts as vectors ----------------------------------------------------------------

def pack(g, loss=None):
    """[centers 3M | colors 3M | radius M | light_dir 3 | ambient 1 | loss 1] as fp64."""
    parts = [np.asarray(g[k], np.float64).reshape(-1) for k in KEYS]
    parts.append(np.array([0.0 if loss is None else float(loss)]))
    return np.concatenate(parts)


def index_sets(m):
    """Slices of pack()'s vector by name."""
    return {"centers": slice(0, 3 * m), "colors": slice(3 * m, 6 * m), "radius": slice(6 * m, 7 * m),
            "light_dir": slice(7 * m, 7 * m + 3), "ambient": slice(7 * m + 3, 7 * m + 4),
            "loss": slice(7 * m + 4, 7 * m + 5)}


def record_row(g, m, mpad=None):
    """A gradient dict as one partial record of the reduction: [Mpad][8] (gc.xyz, gr, gcol.rgb, 0),
    then 8 scalars (the light direction's three terms, ambient, loss, 0, 0, live flag), fp32."""
    mpad = m if mpad is None else mpad
    rec = np.zeros(mpad * 8 + 8, np.float32)
    body = rec[:mpad * 8].reshape(mpad, 8)
    body[:m, 0:3] = np.asarray(g["centers"]).reshape(m, 3)
    body[:m, 3] = np.asarray(g["radius"]).reshape(m)
    body[:m, 4:7] = np.asarray(g["colors"]).reshape(m, 3)
    rec[mpad * 8:mpad * 8 + 3] = np.asarray(g["light_dir"]).reshape(3)
    rec[mpad * 8 + 3] = np.asarray(g["ambient"]).reshape(-1)[0]
    return rec


def axis_light(axis):
    """The axis-aligned light of length 2 along -axis: (0,0,-2), (0,-2,0) or (-2,0,0). With it
    light_grad returns r / 2 exactly in the two orthogonal components and exactly 0 along it."""
    ld = np.zeros(3, np.float32)
    ld[axis] = -2.0
    return ld
