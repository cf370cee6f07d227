"""Host tests of `druggen_amd.schedule.epoch_schedule` on the CPU generator: the index schedule of the reference's loop
(train.py:302-345: molecule loader and drug loader, both shuffle=True / drop_last=True; a new drug iterator per epoch and
whenever the current one is exhausted)."""
import pytest
import torch

CASES = [(11, 6, 4, 1), (11, 6, 4, 2), (8, 8, 4, 1), (9, None, 3, 1)]      # (n_mol, n_drug, B, world)
EPOCHS, SEED = 3, 5


def _run(n_mol, n_drug, B, world, rank, seed=SEED, epochs=EPOCHS):
    """[epoch][step] -> (mol_idx, drug_idx) of one rank."""
    from druggen_amd.schedule import epoch_schedule
    g = torch.Generator().manual_seed(seed)
    return [list(epoch_schedule(n_mol, n_drug, B, generator=g, device="cpu", world=world, rank=rank)) for _ in range(epochs)]


def _global(n_mol, n_drug, B, world):
    """[epoch][step] -> (mol [B], drug [B]): the ranks' slices joined in rank order."""
    per_rank = [_run(n_mol, n_drug, B, world, r) for r in range(world)]
    return [[tuple(torch.cat([per_rank[r][e][s][k] for r in range(world)]) for k in (0, 1))
             for s in range(len(per_rank[0][e]))] for e in range(EPOCHS)]


def _reference_draws(n_mol, n_drug, B):
    """The loop of train.py:302-316 restated on bare permutations: per epoch the drug permutation, the molecule
    permutation, and a new drug permutation whenever fewer than B of the current one remain.  [epoch][step] ->
    (mol list, drug list, index of the drug permutation in use)."""
    g = torch.Generator().manual_seed(SEED)
    out, n_perm = [], 0
    for _ in range(EPOCHS):
        if n_drug is not None:
            drugs, used, n_perm = torch.randperm(n_drug, generator=g).tolist(), 0, n_perm + 1
        mols = torch.randperm(n_mol, generator=g).tolist()
        steps = []
        for s in range(n_mol // B):
            mol = mols[s * B:(s + 1) * B]
            if n_drug is None:
                steps.append((mol, mol, 0))
                continue
            if n_drug - used < B:
                drugs, used, n_perm = torch.randperm(n_drug, generator=g).tolist(), 0, n_perm + 1
            steps.append((mol, drugs[used:used + B], n_perm))
            used += B
        out.append(steps)
    return out


@pytest.mark.parametrize("n_mol,n_drug,B,world", CASES)
def test_molecules_are_a_dropped_prefix_of_one_permutation_per_epoch(n_mol, n_drug, B, world):
    epochs = _global(n_mol, n_drug, B, world)
    seen = []
    for steps in epochs:
        assert len(steps) == n_mol // B
        for mol, drug in steps:
            assert mol.dtype == drug.dtype == torch.int64 and mol.shape == drug.shape == (B,)
        flat = torch.cat([mol for mol, _ in steps]).tolist()
        assert len(flat) == (n_mol // B) * B and len(set(flat)) == len(flat) and set(flat) <= set(range(n_mol))
        seen.append(flat)
    assert seen[0] != seen[1] and seen[1] != seen[2] and seen[0] != seen[2]
    want = _reference_draws(n_mol, n_drug, B)
    assert seen == [[i for mol, _, _ in steps for i in mol] for steps in want]      # a PREFIX of randperm(n_mol), in order


@pytest.mark.parametrize("n_mol,n_drug,B,world", [c for c in CASES if c[1] is not None])
def test_drug_permutation_restarts_at_every_epoch_and_when_exhausted(n_mol, n_drug, B, world):
    epochs = _global(n_mol, n_drug, B, world)
    want = _reference_draws(n_mol, n_drug, B)
    per_perm = {}
    for e, steps in enumerate(epochs):
        assert want[e][0][2] != (want[e - 1][-1][2] if e else 0)                    # a new permutation at the epoch's start
        for s, (_, drug) in enumerate(steps):
            assert 0 <= int(drug.min()) and int(drug.max()) < n_drug
            assert drug.tolist() == want[e][s][1]
            per_perm.setdefault(want[e][s][2], []).extend(drug.tolist())
    for idx in per_perm.values():                                                   # within one permutation nothing repeats,
        assert len(set(idx)) == len(idx) <= (n_drug // B) * B                       # and it serves n_drug // B batches at most
    restarts = [want[e][s][2] != want[e][s - 1][2] for e in range(EPOCHS) for s in range(1, len(want[e]))]
    if (n_mol, n_drug, B) == (11, 6, 4):
        assert all(restarts)          # one drug batch per permutation: every step after an epoch's first restarts
    if (n_mol, n_drug, B) == (8, 8, 4):
        assert not any(restarts)      # two drug batches per permutation, two steps per epoch: only the epoch restarts


def test_no_target_yields_one_tensor_for_both_sides():
    for steps in _run(9, None, 3, 1, 0):
        assert len(steps) == 3
        for mol, drug in steps:
            assert drug is mol


@pytest.mark.parametrize("n_mol,n_drug,B,world", CASES)
def test_same_seed_same_schedule_and_ranks_partition_the_global_batch(n_mol, n_drug, B, world):
    one, again, other = _run(n_mol, n_drug, B, 1, 0), _run(n_mol, n_drug, B, 1, 0), _run(n_mol, n_drug, B, 1, 0, seed=SEED + 1)
    same = lambda p, q: all(torch.equal(a[k], b[k]) for x, y in zip(p, q) for a, b in zip(x, y) for k in (0, 1))
    assert same(one, again) and not same(one, other)
    joined = _global(n_mol, n_drug, B, world)
    assert same(one, joined)                                                        # row for row the world = 1 schedule
    per = B // world
    for r in range(world):
        for e, steps in enumerate(_run(n_mol, n_drug, B, world, r)):
            for s, (mol, drug) in enumerate(steps):
                assert mol.shape == (per,)
                assert torch.equal(mol, one[e][s][0][r * per:(r + 1) * per])
                assert torch.equal(drug, one[e][s][1][r * per:(r + 1) * per])


@pytest.mark.parametrize("args,match", [((11, 6, 4, 3), "multiple"), ((3, 6, 4, 1), "molecules"), ((11, 3, 4, 1), "drugs")])
def test_value_errors_fire_before_anything_is_drawn(args, match):
    from druggen_amd.schedule import epoch_schedule
    n_mol, n_drug, B, world = args
    g = torch.Generator().manual_seed(SEED)
    before = g.get_state()
    with pytest.raises(ValueError, match=match):
        epoch_schedule(n_mol, n_drug, B, generator=g, device="cpu", world=world, rank=0)      # at the call, not at next()
    assert torch.equal(g.get_state(), before)
