"""Seeded fingerprint sets for the Tanimoto tests (tests/test_metrics_host.py, tests/test_hip_metrics.py) and for the
golden fixture tests/golden/tanimoto_ref.npz: dense uint8 0/1 rows, every row with its own density."""
import hashlib

import numpy as np

SEED = 20261017
STOCK, GEN, SELF, NBITS = 6001, 5003, 3000, 1024      # both sizes cross the reference's 5000-row block edge


def random_bits(rng, n, nbits, lo=0.02, hi=0.08):
    """[n, nbits] uint8: row i has every bit set with probability d_i, d_i uniform in [lo, hi)."""
    density = rng.uniform(lo, hi, size=(n, 1))
    return (rng.random((n, nbits)) < density).astype(np.uint8)


def default_case():
    """stock [6001, 1024], gen [5003, 1024], self [3000, 1024]: gen[7] and stock[11] are empty, gen[100] = stock[200]."""
    rng = np.random.default_rng(SEED)
    stock = random_bits(rng, STOCK, NBITS)
    gen = random_bits(rng, GEN, NBITS)
    own = random_bits(rng, SELF, NBITS)
    gen[7] = 0
    stock[11] = 0
    gen[100] = stock[200]
    return {"stock": stock, "gen": gen, "self": own}


def pack_host(x):
    """np.packbits(bitorder='little') read as little-endian uint32: the packed layout, written here independently of the product."""
    return np.ascontiguousarray(np.packbits(np.asarray(x) != 0, axis=1, bitorder="little")).view("<u4")


def input_hash(case):
    h = hashlib.sha256()
    for name in ("stock", "gen", "self"):
        h.update(pack_host(case[name]).astype("<u4").tobytes())
    return h.hexdigest()


def shape_case(S, G, nbits, seed, lo=0.02, hi=0.5):
    rng = np.random.default_rng(seed)
    return random_bits(rng, S, nbits, lo, hi), random_bits(rng, G, nbits, lo, hi)
