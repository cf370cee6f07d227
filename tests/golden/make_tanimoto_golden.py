"""Writes tests/golden/tanimoto_ref.npz: what the REFERENCE's `average_agg_tanimoto` / `internal_diversity`
(src/util/utils.py) return on the seeded inputs of tests/tanimoto_cases.py.  Runs only where the reference checkout is
present; the two functions are taken out of utils.py by name with `ast` (the module itself imports RDKit) and executed
with numpy and torch in scope.  The fixture holds their outputs, a hash of the packed inputs and the seed.

    python tests/golden/make_tanimoto_golden.py /path/to/reference
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tanimoto_cases  # noqa: E402

NAMES = ("average_agg_tanimoto", "internal_diversity")


def load_reference(root):
    path = os.path.join(root, "src", "util", "utils.py")
    tree = ast.parse(open(path).read())
    picked = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    assert sorted(n.name for n in picked) == sorted(NAMES), [n.name for n in picked]
    scope = {"np": np, "torch": torch}
    exec(compile(ast.Module(body=picked, type_ignores=[]), path, "exec"), scope)
    return scope


def main():
    ref = load_reference(sys.argv[1])
    case = tanimoto_cases.default_case()
    agg = ref["average_agg_tanimoto"]
    stock, gen = case["stock"], case["gen"]
    out = {
        "max": agg(stock, gen, agg="max", intdiv=True),
        "mean": agg(stock, gen, agg="mean", intdiv=True),
        "snn": np.float64(agg(stock, gen, agg="max")),
        "intdiv": np.array(ref["internal_diversity"](case["self"]), dtype=np.float64),
        "seed": np.int64(tanimoto_cases.SEED),
        "sha256": np.array(tanimoto_cases.input_hash(case)),
    }
    np.savez_compressed(os.path.join(HERE, "tanimoto_ref.npz"), **out)
    print({k: (v.shape, v.dtype) for k, v in out.items()}, out["snn"], out["intdiv"])


if __name__ == "__main__":
    main()
