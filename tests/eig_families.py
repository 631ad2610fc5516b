"""Input families for the symmetric-eigensolver tests, the bars those tests assert, and T_d methane.  numpy only; deterministic.

family(name, n, seed) -> A (n, n), symmetric.  Unless stated, A = Q diag(d) Q^T symmetrised with Q from a seeded QR and d = spectrum(name,
n, seed).  Each family is aimed at one mechanism of the cold eigensolve (Householder start, multisection, twisted factorisation, refinement
rule, hand-over to rotations):

  dense       0.5 (G + G^T), G standard normal: a generic, well separated spectrum (what test_sym_eig feeds)
  pairs       sorted uniform(-10, 10), every third eigenvalue repeated exactly once: benzene-like E-type pairs
  atom        exact multiplicities 1, 3, 5, 7 cycling, level spacings uniform(0.05, 1.5) from -20: shells of an atom
  splits      uniform(-10, 10) with triplets d, d + g, d + 2 g at every 7th index, g cycling through 1e-12 .. 1e-4: in units of the scale
              (10) the splits sit at QC_REF_TINY (1e-13), around the start's perturbation (1e-11) and around QC_REF_GFLOOR (1e-8)
  core        {-105, -10.6, -8.07, -8.07, -8.07} + sorted uniform(-1.2, 4.0): a Cl-like scale over a dense valence band
  lowrank     0.7 I + U diag(1, 2, -3) U^T / n, U standard normal (n, 3): one eigenvalue of multiplicity n - 3 (built directly)
  blocks      block-diagonal, random symmetric blocks of sizes 1..39, exact zeros elsewhere (built directly): a Householder step meets a
              zero column, the tridiagonal matrix has exact zeros in e
  permblocks  blocks under a seeded symmetric permutation: reducible, but not visibly so
  diag        diag(uniform(-10, 10)): every Householder step is the identity
  tridiag     that diagonal plus uniform(-1, 1) off-diagonals: already reduced
  wilkinson   W_n^+: diagonal |i - (n - 1) / 2|, off-diagonals 1; its top eigenvalues pair up to ~1e-15 relative without being equal
  const       CONST_VALUES[seed % 2] * I: 0.7 I and the zero matrix (n = 24 and 65 only: the result must be finite and within the bars)

bars(n, w_ref) -> (eigenvalue, orthogonality, residual) bounds; errors(A, V, w, w_ref) -> the three figures they bound.
warm_case(name, n, eps) -> (B, V0): the input of a warm eigensolve, B = A + eps (P + P^T) with V0 the eigenvectors of A.
methane(basis_name) -> MolecularSystem of T_d methane."""
import os

import numpy as np

FAMILIES = ("dense", "pairs", "atom", "splits", "core", "lowrank", "blocks", "permblocks", "diag", "tridiag", "wilkinson")
SPECTRAL = ("pairs", "atom", "splits", "core")           # built as Q diag(spectrum) Q^T
CONST_VALUES = (0.7, 0.0)
SPLIT_STRIDE = 7
SPLIT_GAPS = tuple(10.0 ** k for k in range(-12, -3))     # 1e-12 .. 1e-4
ATOM_MULT = (1, 3, 5, 7)
CORE_LEVELS = (-105.0, -10.6, -8.07, -8.07, -8.07)
BLOCK_MAX = 39


def _rng(name, n, seed):
    return np.random.default_rng([FAMILIES.index(name) if name in FAMILIES else len(FAMILIES), n, seed])


def rand_sym(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    return 0.5 * (A + A.T)


def split_starts(n):
    """first index of every triplet of `splits`"""
    return list(range(0, n - 2, SPLIT_STRIDE))


def spectrum(name, n, seed):
    """the eigenvalues a SPECTRAL family is built from (not sorted for `splits`)"""
    rng = _rng(name, n, seed)
    if name == "pairs":
        d = np.sort(rng.uniform(-10, 10, n))
        d[1::3] = d[0:n - 1:3]
        return d
    if name == "atom":
        d, level, k = [], -20.0, 0
        while len(d) < n:
            d += [level] * ATOM_MULT[k % len(ATOM_MULT)]
            level += rng.uniform(0.05, 1.5)
            k += 1
        return np.array(d[:n])
    if name == "splits":
        d = np.sort(rng.uniform(-10, 10, n))
        for t, i in enumerate(split_starts(n)):
            g = SPLIT_GAPS[t % len(SPLIT_GAPS)]
            d[i + 1] = d[i] + g
            d[i + 2] = d[i] + 2 * g
        return d
    if name == "core":
        return np.concatenate([CORE_LEVELS, np.sort(rng.uniform(-1.2, 4.0, n - len(CORE_LEVELS)))])
    raise KeyError(name)


def block_sizes(n, seed):
    rng = _rng("blocks", n, seed)
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(int(rng.integers(1, BLOCK_MAX + 1)), n - sum(sizes)))
    return sizes


def _blocks(n, seed):
    A = np.zeros((n, n))
    at = 0
    for k, b in enumerate(block_sizes(n, seed)):
        A[at:at + b, at:at + b] = rand_sym(b, [n, seed, k])
        at += b
    return A


def permutation(n, seed):
    return _rng("permblocks", n, seed).permutation(n)


def family(name, n, seed):
    if name == "dense":
        return rand_sym(n, seed)
    if name in SPECTRAL:
        d = spectrum(name, n, seed)
        Q, _ = np.linalg.qr(_rng(name, n, seed + 1).standard_normal((n, n)))
        A = (Q * d) @ Q.T
        return 0.5 * (A + A.T)
    if name == "lowrank":
        U = _rng(name, n, seed).standard_normal((n, 3))
        A = 0.7 * np.eye(n) + (U * np.array([1.0, 2.0, -3.0])) @ U.T / n
        return 0.5 * (A + A.T)
    if name == "blocks":
        return _blocks(n, seed)
    if name == "permblocks":
        p = permutation(n, seed)
        return np.ascontiguousarray(_blocks(n, seed)[np.ix_(p, p)])
    if name in ("diag", "tridiag"):
        rng = _rng("diag", n, seed)                       # (tridiag: the same diagonal)
        A = np.diag(rng.uniform(-10, 10, n))
        if name == "tridiag":
            e = rng.uniform(-1, 1, n - 1)
            A += np.diag(e, 1) + np.diag(e, -1)
        return A
    if name == "wilkinson":
        return np.diag(np.abs(np.arange(n) - 0.5 * (n - 1))) + np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)
    if name == "const":
        return CONST_VALUES[seed % 2] * np.eye(n)
    raise KeyError(name)


def bars(n, w_ref):
    """Bounds on max|w - w_ref|, max|V^T V - I| and max|A V - V w|.  With f = max(1, n / 230) and s = max(1, max|w_ref|): 1e-12 f s, 1e-12 f,
    1e-11 f s - at n <= 230 the numbers test_sym_eig asserts, growing linearly above: the backward error of an orthogonal-transformation
    eigensolver finished by GEMM refinement is a low-degree polynomial in n times eps ||A|| (reflections and inner products of length n
    contribute O(n eps) each)."""
    f = max(1.0, n / 230.0)
    s = max(1.0, float(np.abs(w_ref).max()))
    return 1e-12 * f * s, 1e-12 * f, 1e-11 * f * s


def errors(A, V, w, w_ref):
    n = len(w)
    return float(np.abs(w - w_ref).max()), float(np.abs(V.T @ V - np.eye(n)).max()), float(np.abs(A @ V - V * w).max())


def check(A, V, w, margin=1.0, label=None):
    """the assertions of every eigensolver case: finite, ascending, the three bars (each figure is printed first when a label is given)"""
    n = A.shape[0]
    assert np.all(np.isfinite(V)) and np.all(np.isfinite(w)), label
    w_ref = np.linalg.eigvalsh(A)
    err, bar = errors(A, V, w, w_ref), bars(n, w_ref)
    if label:
        print("EIG %-28s n %3d  dw %.2e / %.2e  orth %.2e / %.2e  res %.2e / %.2e" % (label, n, err[0], bar[0], err[1], bar[1], err[2], bar[2]))
    assert np.all(np.diff(w) >= 0), "eigenvalues not ascending"
    for what, e, b in zip(("eigenvalues", "orthogonality", "residual"), err, bar):
        assert e * margin < b, f"{what}: {e:.3e} (x{margin:g}) against {b:.3e} at n = {n}"
    return err, bar


def warm_case(name, n, eps, seed=None):
    A = family(name, n, n if seed is None else seed)
    _, V0 = np.linalg.eigh(A)
    P = _rng(name, n, 7919).standard_normal((n, n))
    return A + eps * (P + P.T), V0


METHANE_CH = 2.0598                                       # bohr
METHANE_H = ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))


def methane_atoms():
    """[(Z, position)]: C at the origin, four H at a (+-1, +-1, +-1) with an even number of minus signs, a = 2.0598 / sqrt 3 bohr (T_d)"""
    a = METHANE_CH / np.sqrt(3.0)
    return [(6, (0.0, 0.0, 0.0))] + [(1, tuple(a * c for c in h)) for h in METHANE_H]


def methane(basis_name):
    import qchem_rs_amd as q
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    basis = q.BasisSet.load(os.path.join(root, "data", "basis", basis_name + ".json"))
    return q.MolecularSystem.from_atoms([q.Atom(z, list(r)) for z, r in methane_atoms()], basis)
