"""The inputs of tests/test_eigensolver_gpu.py, checked on the CPU: every family of eig_families.py has the property it is named for, and
LAPACK (np.linalg.eigh) meets every bar of eig_families.bars with a margin of 100 at every size the GPU tests use - so a bar missed on
the GPU is the product's error, not the input's conditioning or the reference's own.  The margin is a condition on the inputs: a family
that cannot meet it is changed, not the margin."""
import numpy as np
import pytest

import eig_families as ef

SIZES_ALL = (24, 58, 64, 65, 128, 129, 192, 193, 257, 512)                  # cold entry, every family
SIZES_NEW = (256, 257, 320, 321, 384, 385, 448, 449, 512, 513)              # cold entry, dense and atom
SIZES_ROUTE = (24, 58, 114, 257, 512)                                       # which layer answered, dense and pairs
MARGIN = 100.0


def _eigh_meets_the_bars(A):
    w, V = np.linalg.eigh(A)
    return ef.check(A, V, w, margin=MARGIN)


@pytest.mark.parametrize("n", SIZES_ALL)
def test_lapack_meets_the_bars_with_margin_every_family(n):
    for name in ef.FAMILIES:
        A = ef.family(name, n, n)
        assert A.shape == (n, n) and np.array_equal(A, A.T), name
        assert np.array_equal(A, ef.family(name, n, n)), name                # deterministic
        _eigh_meets_the_bars(A)


@pytest.mark.parametrize("n", sorted(set(SIZES_NEW + SIZES_ROUTE) - set(SIZES_ALL)))
def test_lapack_meets_the_bars_with_margin_new_sizes(n):
    for name in ("dense", "atom", "pairs"):
        _eigh_meets_the_bars(ef.family(name, n, n))


@pytest.mark.parametrize("n", (24, 65))
def test_const_is_a_multiple_of_the_identity(n):
    for seed, c in enumerate(ef.CONST_VALUES):
        A = ef.family("const", n, seed)
        assert np.array_equal(A, c * np.eye(n))
        _eigh_meets_the_bars(A)
    assert ef.CONST_VALUES == (0.7, 0.0)


@pytest.mark.parametrize("n", (257, 512))
@pytest.mark.parametrize("name", ("atom", "splits"))
def test_lapack_meets_the_bars_on_the_warm_inputs(name, n):
    for eps in (0.0, 1e-9, 1e-3, 0.3):
        B, V0 = ef.warm_case(name, n, eps)
        assert np.abs(V0.T @ V0 - np.eye(n)).max() < 1e-13
        assert float(np.abs(np.linalg.eigvalsh(B)).max()) < 300.0            # the norm range of an SCF
        _eigh_meets_the_bars(B)


def test_dense_is_the_matrix_of_test_sym_eig():
    rng = np.random.default_rng(58)
    G = rng.standard_normal((58, 58))
    assert np.array_equal(ef.family("dense", 58, 58), 0.5 * (G + G.T))


@pytest.mark.parametrize("n", (24, 58, 257, 512))
def test_pairs_repeats_every_third_eigenvalue_exactly_once(n):
    d = ef.spectrum("pairs", n, n)
    assert np.all(np.diff(d) >= 0) and np.abs(d).max() < 10
    same = np.diff(d) == 0.0
    assert np.array_equal(np.flatnonzero(same), np.arange(0, n - 1, 3))      # d[3k] == d[3k + 1] and no other repeat
    # the matrix keeps the pairs to rounding, far below the start's perturbation (1e-11 of the scale)
    w = np.linalg.eigvalsh(ef.family("pairs", n, n))
    assert np.abs(w - d).max() < 1e-13 * 10 and np.diff(w)[same].max() < 1e-13 * 10


@pytest.mark.parametrize("n", (24, 65, 257, 512))
def test_atom_has_multiplicities_1_3_5_7(n):
    d = ef.spectrum("atom", n, n)
    assert d[0] == -20.0 and len(d) == n
    levels, counts = np.unique(d, return_counts=True)
    want = [ef.ATOM_MULT[k % 4] for k in range(len(levels))]
    assert list(counts[:-1]) == want[:-1] and 1 <= counts[-1] <= want[-1]   # (the last level is cut off at n)
    gaps = np.diff(levels)
    assert gaps.min() >= 0.05 and gaps.max() <= 1.5
    assert np.abs(d).max() < 300.0
    w = np.linalg.eigvalsh(ef.family("atom", n, n))
    assert np.abs(w - d).max() < 1e-13 * np.abs(d).max()


@pytest.mark.parametrize("n", (24, 64, 257, 512))
def test_splits_sit_on_the_intended_sides_of_the_thresholds(n):
    """With s = max|d| (just under 10): g = 1e-12 is at QC_REF_TINY s (1e-13 s), 1e-12 and 1e-11 are below the start's perturbation
    (1e-11 s), 1e-10 is at it, the rest above; 1e-12 .. 1e-8 are below QC_REF_GFLOOR s (1e-8 s), 1e-7 is at it, 1e-6 .. 1e-4 above.  `At`:
    within [1, 2) times the threshold."""
    d = ef.spectrum("splits", n, n)
    s = np.abs(d).max()
    assert 8.0 < s < 10.0 + 2e-4
    starts = ef.split_starts(n)
    assert len(starts) >= min(9, (n - 2 + 6) // 7)
    seen = set()
    for t, i in enumerate(starts):
        k = t % len(ef.SPLIT_GAPS)
        g = ef.SPLIT_GAPS[k]
        seen.add(k)
        for got in (d[i + 1] - d[i], d[i + 2] - d[i + 1]):
            assert abs(got - g) <= 4e-15 + 1e-9 * g                           # (spacing of doubles near 10: 1.8e-15)
            if k >= 1:
                # the smallest split lies within rounding of its nominal size only; the others to better than 1 %
                assert abs(got - g) < 1e-2 * g
        tiny, pert, gfloor = 1e-13 * s, 1e-11 * s, 1e-8 * s
        assert (1.0 <= g / tiny < 2.0) if k == 0 else g > 5 * tiny
        assert (g < pert / 5) if k < 2 else ((1.0 <= g / pert < 2.0) if k == 2 else g > 5 * pert)
        assert (g < gfloor / 5) if k < 5 else ((1.0 <= g / gfloor < 2.0) if k == 5 else g > 5 * gfloor)
    assert seen == set(range(min(len(starts), len(ef.SPLIT_GAPS))))
    if n >= 64:
        assert len(seen) == 9                                                 # every size from 1e-12 to 1e-4 occurs


@pytest.mark.parametrize("n", (24, 257, 512))
def test_core_has_a_deep_level_a_triple_and_a_dense_band(n):
    d = ef.spectrum("core", n, n)
    assert tuple(d[:5]) == (-105.0, -10.6, -8.07, -8.07, -8.07)
    band = d[5:]
    assert np.all(np.diff(band) > 0) and band.min() >= -1.2 and band.max() <= 4.0
    assert np.abs(d).max() == 105.0
    if n == 512:
        assert 1e-5 < np.median(np.diff(band)) / 105.0 < 1e-4 * 1.5             # gaps ~1e-4 of the scale


@pytest.mark.parametrize("n", (24, 65, 512))
def test_lowrank_has_one_eigenvalue_of_multiplicity_n_minus_3(n):
    A = ef.family("lowrank", n, n)
    w = np.linalg.eigvalsh(A)
    assert np.linalg.matrix_rank(A - 0.7 * np.eye(n), tol=1e-12) == 3
    assert np.sum(np.abs(w - 0.7) < 1e-14) == n - 3
    assert np.sum(w > 0.7 + 0.1) == 2 and np.sum(w < 0.7 - 0.1) == 1


@pytest.mark.parametrize("n", (24, 65, 257, 512))
def test_blocks_are_exactly_reducible(n):
    sizes = ef.block_sizes(n, n)
    assert sum(sizes) == n and 1 <= min(sizes) and max(sizes) <= ef.BLOCK_MAX and len(sizes) >= 2
    A = ef.family("blocks", n, n)
    mask = np.zeros((n, n), bool)
    at = 0
    for b in sizes:
        mask[at:at + b, at:at + b] = True
        at += b
    assert np.all(A[~mask] == 0.0) and np.all(A[mask] != 0.0)
    P = ef.family("permblocks", n, n)
    p = ef.permutation(n, n)
    assert np.array_equal(P, A[np.ix_(p, p)]) and np.array_equal(np.sort(p), np.arange(n))
    assert np.count_nonzero(P) == np.count_nonzero(A) and not np.array_equal(P, A)
    assert np.abs(np.linalg.eigvalsh(P) - np.linalg.eigvalsh(A)).max() < 1e-13 * 10


@pytest.mark.parametrize("n", (24, 65, 512))
def test_diag_tridiag_and_wilkinson(n):
    D, T, W = (ef.family(name, n, n) for name in ("diag", "tridiag", "wilkinson"))
    off = ~np.eye(n, dtype=bool)
    assert np.all(D[off] == 0.0) and np.abs(np.diag(D)).max() < 10 and len(np.unique(np.diag(D))) == n
    assert np.array_equal(np.diag(T), np.diag(D))
    band = np.abs(np.subtract.outer(np.arange(n), np.arange(n))) <= 1
    assert np.all(T[~band] == 0.0) and np.all(np.diag(T, 1) != 0.0) and np.abs(np.diag(T, 1)).max() < 1
    assert np.array_equal(np.diag(W), np.abs(np.arange(n) - 0.5 * (n - 1)))
    assert np.all(np.diag(W, 1) == 1.0) and np.all(W[~band] == 0.0)
    w = np.linalg.eigvalsh(W)
    assert w[-1] < 300.0
    assert 0.0 <= w[-1] - w[-2] < 1e-13 * w[-1]                               # the top pair agrees to rounding (and is not equal in exact arithmetic)


def test_methane_is_tetrahedral():
    atoms = ef.methane_atoms()
    assert [z for z, _ in atoms] == [6, 1, 1, 1, 1] and atoms[0][1] == (0.0, 0.0, 0.0)
    H = np.array([r for _, r in atoms[1:]])
    assert np.allclose(np.linalg.norm(H, axis=1), 2.0598, rtol=0, atol=1e-15)
    hh = [np.linalg.norm(H[i] - H[j]) for i in range(4) for j in range(i)]
    assert np.allclose(hh, 2.0598 * np.sqrt(8.0 / 3.0), rtol=0, atol=1e-14)
    assert np.abs(H.sum(axis=0)).max() < 1e-15
    assert [ef.methane(b).n_basis() for b in ("6-31G_st_st", "cc-pVDZ", "cc-pVTZ")] == [35, 34, 86]
