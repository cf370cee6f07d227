"""Exact numpy restatement of `dg_fp_tanimoto` (include/druggen_hip.h), written from its definition: integer
intersections c and bit counts a, b; q = float32(c) / float32(a + b - c), 1 where the denominator is 0;
max over the stock with the first index on ties; the mean as the float64 sum of the float32 quotients over S; and the
exact mean, every quotient in float64."""
import numpy as np


def intersections(stock, gen):
    """[S, G] int64 = |stock_s & gen_g|.  The float64 matrix product of 0/1 values is exact (counts <= 4096 << 2^53)."""
    return np.rint((stock != 0).astype(np.float64) @ (gen != 0).astype(np.float64).T).astype(np.int64)


def aggregate(stock, gen, block=512):
    """-> dict(max float32 [G], idx int64 [G], mean float64 [G], exact_mean float64 [G])."""
    stock, gen = np.asarray(stock), np.asarray(gen)
    S, G = len(stock), len(gen)
    a = (stock != 0).sum(1).astype(np.int64)
    out = {"max": np.zeros(G, np.float32), "idx": np.zeros(G, np.int64), "mean": np.zeros(G), "exact_mean": np.zeros(G)}
    for g0 in range(0, G, block):
        part = gen[g0:g0 + block]
        b = (part != 0).sum(1).astype(np.int64)
        c = intersections(stock, part)
        d = a[:, None] + b[None, :] - c
        zero = d == 0
        cs, ds = np.where(zero, 1, c), np.where(zero, 1, d)
        q32 = cs.astype(np.float32) / ds.astype(np.float32)          # IEEE float32 division, correctly rounded
        sl = slice(g0, g0 + len(part))
        out["max"][sl] = q32.max(0)
        out["idx"][sl] = q32.argmax(0)                                # first maximum
        out["mean"][sl] = q32.astype(np.float64).sum(0) / S
        out["exact_mean"][sl] = (cs.astype(np.float64) / ds.astype(np.float64)).sum(0) / S
    return out
