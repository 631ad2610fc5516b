"""The symmetric eigensolver (qc_eig_tridiag.hip, qc_eig_refine.hip with qc_refine_rule.h, qc_eig_jacobi.hip) on what it is built for:
the whole supported size range of the cold entry (24..512, and 513, the first size that goes to qc_jacobi1g_kernel), degenerate, clustered
and reducible input (tests/eig_families.py), the warm entry above n = 230, and T_d methane through the SCF drivers.

Bars (eig_families.bars; stated, not measured): w ascending, max|w - w_ref| < 1e-12 f s, max|V^T V - I| < 1e-12 f, max|A V - V w| < 1e-11 f s
with f = max(1, n / 230), s = max(1, max|w_ref|), w_ref from np.linalg.eigvalsh.  tests/test_eig_families_host.py shows that LAPACK meets
them with a margin of 100 on every input used here.

MEASURED (MI355X; per regime the case with the largest error / bar, as error of bar, family n).  Eigenvalue errors of 1e-11 come from
the one-sided Jacobi kernels (w = ||g|| - sigma with a Gershgorin shift sigma of ~sqrt(n) ||A||), everything else sits at rounding:
  regime                     eigenvalues                        orthogonality                      residual
  cold, n = 24..64           9.8e-13 of 1.0e-11, splits 58      2.7e-14 of 1.0e-12, atom 64        3.0e-12 of 9.9e-11, splits 64
  cold, n = 65..128          4.2e-12 of 2.0e-11, atom 128       2.6e-14 of 1.0e-12, atom 65        3.1e-12 of 1.6e-10, dense 128
  cold, n = 129..192         6.6e-12 of 2.0e-11, atom 192       1.7e-15 of 1.0e-12, lowrank 192    3.5e-11 of 9.6e-10, wilkinson 192
  cold, n = 193..256         1.5e-11 of 3.4e-11, atom 256       1.8e-15 of 1.0e-12, core 193       4.1e-12 of 2.0e-10, dense 193
  cold, n = 257..512         1.0e-11 of 2.2e-11, splits 512     2.2e-15 of 1.1e-12, pairs 257      5.3e-12 of 2.5e-10, dense 257
  cold, n = 513              2.6e-11 of 7.2e-11, dense 513      2.2e-15 of 2.2e-12, dense 513      1.0e-11 of 1.7e-09, atom 513
  warm entry, n = 257, 512   9.6e-12 of 2.2e-11, pairs 512 (I)  3.3e-15 of 1.1e-12, atom 257       1.6e-12 of 2.2e-10, pairs 512 (I)
Before the Jacobi kernels looked at what a sweep leaves (QC_JACOBI_LEFT_TOL, qc_internal.h) these cases missed their bars: residual
3.7e-10 (pairs 58) and 4.4e-10 (atom 64) from the two-sided kernel, orthogonality 1.6e-12 (atom 128) from the one-sided LDS kernel and
1.3e-11 .. 2.2e-11 (atom 193, 256, 257, 321, 385) from the global-memory one, 1.7e-11 / 1.3e-10 with eigenvalues 2.1e-10 off on the warm
entry (atom 257 / 512, eps 1e-9), and methane/cc-pVTZ's orbital energies were 1.2e-9 off with a triple 2.3e-9 wide.  The slowest cases
take 0.8 s (n = 512, 513 through qc_jacobi1g_kernel), the child process of the route test 3.5 s.

ROUTES (state of the cold entry's control word: 1 = QC_EIG_DONE, the tridiagonal start + refinement answered, in `passes` passes;
2 = QC_EIG_ROTATE, the eigensolve was repeated by the Jacobi kernels: a second eigensolve, 0.1 s at n = 256, 0.8 s at 512).  Asserted for
dense and for pairs at 24 (test_which_layer_answered says why not above); the rest as seen in the whole run, by size:
  family      24    58    64    65    128   129   192   193   257   512   (114 for dense, pairs: 1 / 2)
  dense       1     1     1     1     1     1     1     1     1     1     also 256..512 of the first test
  pairs       1     2     1     1     2     2     2     2     2     2
  atom        1     2     2     2     2     2     2     2     2     2     also 256..512 of the first test
  splits      2     1     1     1     1     1     2     2     2     2
  core        1     1     1     1     1     1     1     2     2     2
  lowrank     1     2     2     2     2     2     2     2     2     2
  blocks, permblocks, diag, tridiag   1 at every size, one pass
  wilkinson   2     2     2     2     2     2     1     2     1     1
  const       0.7 I: 1 at 24, 2 at 65; zero matrix: 2 at both

What these cases do NOT detect is a start that is merely worse: scratch builds without the perturbation, with eight multisection rounds
and with the t == 0 branch of the Householder kernels forced through the update (a no-op: v = e_{k+1}, p = 0) pass every bar on pairs, atom,
blocks, permblocks and tridiag at all ten sizes - the refinement's control word catches the worse start, and 20, 19 and 16 of those 50
cases go on to rotations instead of 16 (pairs at 24 among them, which test_which_layer_answered then reports).  "Correctness never rests on
qc_eig_tridiag.hip" holds; what the start buys is the second eigensolve it saves.

METHANE (passes to 1e-10, counters()["redos"] = passes whose eigensolve was repeated, largest deviations at convergence):
  6-31G**  n 35  14 passes  redos 8   |dD| 2.4e-11  |dw| 6.7e-12  widest triple 6.0e-12   (from the oracle's guess, see GUESS_NOT_UNIQUE)
  cc-pVDZ  n 34  13 passes  redos 0   |dD| 1.8e-11  |dw| 1.1e-11  widest triple 2.1e-11
  cc-pVTZ  n 86  14 passes  redos 7   |dD| 1.3e-11  |dw| 6.8e-11  widest triple 6.1e-12
  UHF (5, 5) cc-pVDZ: 11 passes, E - E_RHF = -1.2e-10
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_system
import eig_families as ef

pytestmark = pytest.mark.gpu

TOL_E = 1e-8
SIZES_ALL = (24, 58, 64, 65, 128, 129, 192, 193, 257, 512)        # both sides of every Householder-kernel switch, one size per new regime
SIZES_NEW = (256, 257, 320, 321, 384, 385, 448, 449, 512)          # both sides of every switch of the back-transformation instance
ROUTE_SIZES = (24, 58, 114, 257, 512)
ROUTE_ASSERTED = [("dense", n) for n in ROUTE_SIZES] + [("pairs", 24)]      # where the start + refinement must answer (see the test)
ROUTE_RECORDED = [("pairs", n) for n in ROUTE_SIZES[1:]] + [(name, n) for name in ef.FAMILIES if name not in ("dense", "pairs") for n in (58, 257)]
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def handle():
    import qchem_rs_amd as q
    s = q.System(load_system("hydrogen", "STO-3G"))
    yield s
    s.close()


@pytest.mark.parametrize("n", SIZES_NEW + (513,))
@pytest.mark.parametrize("name", ("dense", "atom"))
def test_cold_entry_at_the_new_sizes(handle, name, n):
    """n = 257..512: qc_tridiag_kernel<false> (matrix in global memory), qc_backtransform_kernel<5..8> (28-row LDS chunks at 512), the
    chip-wide refinement kernels; n = 513: the hand-over of the cold entry to qc_jacobi1g_kernel."""
    A = ef.family(name, n, n)
    V, w = handle.sym_eig(A)
    ef.check(A, V, w, label=f"cold {name}")


@pytest.mark.parametrize("n", SIZES_ALL)
@pytest.mark.parametrize("name", ef.FAMILIES)
def test_cold_entry_every_family(handle, name, n):
    A = ef.family(name, n, n)
    V, w = handle.sym_eig(A)
    ef.check(A, V, w, label=f"cold {name}")


@pytest.mark.parametrize("n", (24, 65))
@pytest.mark.parametrize("which", (0, 1))
def test_cold_entry_multiple_of_the_identity(handle, which, n):
    """0.7 I and the zero matrix: every eigenvalue equal, every vector an eigenvector (QC_REF_SCALE_FLOOR exists for the zero matrix)"""
    A = ef.family("const", n, which)
    V, w = handle.sym_eig(A)
    ef.check(A, V, w, label=f"cold const {ef.CONST_VALUES[which]}")


@pytest.mark.parametrize("n", (257, 512))
@pytest.mark.parametrize("name", ("atom", "splits"))
def test_warm_entry_above_230(handle, name, n):
    """qc_sym_eig_warm from the eigenvectors of a nearby matrix: exact start, GEMM refinement (1e-9, 1e-3), Jacobi on V0^T B V0 (0.3) - the
    one-workgroup qc_refine_stats_kernel and qc_sort_columns_kernel at n > 230."""
    for eps in (0.0, 1e-9, 1e-3, 0.3):
        B, V0 = ef.warm_case(name, n, eps)
        V, w = handle.sym_eig_warm(B, V0)
        ef.check(B, V, w, label=f"warm {name} eps {eps:g}")


@pytest.mark.parametrize("n", (257, 512))
def test_rotation_kernels_above_230(handle, n):
    """sym_eig_warm(A, I): the refinement finds a dense A far from diagonal and hands it to the rotation kernels (here qc_jacobi1g_kernel)"""
    A = ef.family("pairs", n, n)
    V, w = handle.sym_eig_warm(A, np.eye(n))
    ef.check(A, V, w, label="warm-from-I pairs")


CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2]]
import eig_families as ef
from conftest import load_system
import qchem_rs_amd as q
s = q.System(load_system("hydrogen", "STO-3G"))
for case in sys.argv[3:]:
    name, n = case.split(":")
    sys.stderr.write("[case %s %s]\n" % (name, n)); sys.stderr.flush()
    s.sym_eig(ef.family(name, int(n), int(n)))
s.close()
"""


def test_which_layer_answered():
    """The control word of the cold entry must read QC_EIG_DONE (the tridiagonal start + refinement answered) for dense at every size, and
    for pairs at n = 24.  The header of qc_eig_tridiag.hip used to claim it for exact pairs at every size; it holds only for small n.  The
    1e-11 diagonal perturbation P splits a pair (x_i, x_j) by the eigenvalue difference of the 2 x 2 block x^T P x, ~1e-11 max|a| / sqrt n
    for delocalised vectors: at least 1e-11 at n = 24, 7e-13 at 58, 7e-14 at 114 and 257, 2e-13 at 512 over the pairs of this family,
    median 1e-11 .. 1e-12.  The multisection ends at 65^-9 of the Gershgorin range (2e-15 here), but a Sturm count is only good to a few
    eps max|w| ~ 1e-14, so the twisted vectors of the narrowest pair are mixed by 1e-14 / split: 1e-3 at n = 24, 1e-2 .. 1e-1 from n = 58
    on, above QC_REF_ORTH_LOST (1e-3), and the refinement rightly asks for rotations.  A larger perturbation would leave a coupling inside
    the pair above QC_REF_CLEAN: the thresholds stay, the header and DESIGN 3.4 say what happens.  For pairs above 24 and the other families
    the route is recorded (module docstring), not asserted.  The library reads QC_EIG_DEBUG once per process, hence one fresh child."""
    cases = ROUTE_ASSERTED + ROUTE_RECORDED
    env = dict(os.environ, QC_EIG_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.dirname(HERE), HERE] + [f"{a}:{n}" for a, n in cases],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    routes, case = {}, None
    for line in r.stderr.splitlines():
        m = re.match(r"\[case (\w+) (\d+)\]", line)
        if m:
            case = (m.group(1), int(m.group(2)))
            continue
        m = re.match(r"\[eig cold n=(\d+)\] ctl (\d+) (\d+) (\d+) passes (\d+)", line)
        if m:
            assert case is not None and int(m.group(1)) == case[1] and case not in routes, line
            routes[case] = (int(m.group(2)), int(m.group(5)))
    assert set(routes) == set(cases), sorted(set(cases) - set(routes))
    for case in cases:
        print("ROUTE %-10s n %3d  state %d  passes %d" % (case + routes[case]))
    assert all(routes[c][0] in (1, 2) for c in cases), routes
    assert [c for c in ROUTE_ASSERTED if routes[c][0] != 1] == []


# 6-31G**: the Hueckel guess (rhf.rs:133-150) has the levels -36.49, -16.05, -12.86, then a triple at -11.83 as orbitals 3, 4, 5: the
# occupation (five orbitals) cuts through the triple, so the guess density depends on the basis the eigensolver happens to return inside
# that level, and with it every pass (like O2 in test_startup_stages_match_oracle).  In cc-pVDZ and cc-pVTZ the boundary falls between levels.
GUESS_NOT_UNIQUE = ("6-31G_st_st",)
METHANE_ENERGY = {"6-31G_st_st": -40.2015915835, "cc-pVDZ": -40.1987102895, "cc-pVTZ": -40.2133010044}
_methane_cache = {}


def _methane(basis):
    """(q, System, Oracle, the oracle's converged run with its trace and its ERI tensor); computed once per basis"""
    if basis not in _methane_cache:
        import qchem_rs_amd as q
        from oracle.oracle import Oracle
        m = ef.methane(basis)
        o = Oracle(m)
        I = o.eri()
        ref = o.rhf(100, 1e-10, eri=I, trace=True)
        assert ref["status"] == 0 and abs(ref["total_energy"] - METHANE_ENERGY[basis]) < 1e-9, ref["total_energy"]
        F = o.core_guess()[1] + o.g_rhf(ref["density"], I)
        del I
        X = o.core_guess()[2]
        ref["w_fock"] = np.linalg.eigvalsh(X.T @ F @ X)
        _methane_cache[basis] = (q, m, o, ref)
    return _methane_cache[basis]


@pytest.mark.parametrize("basis,n", [("6-31G_st_st", 35), ("cc-pVDZ", 34), ("cc-pVTZ", 86)])
def test_methane_rhf_passes_and_converged_state(basis, n):
    """T_d methane: three-fold degenerate levels (occupied 1t2, virtual t2 and t1) in every eigensolve of the SCF - the LDS form of the
    refinement inside the one-workgroup kernel (n <= 64) and the generic sequence (n = 86).  Every pass against the oracle's trace with the
    bars of test_rhf_passes_match_oracle_one_by_one; the converged density, tr(D S) = N, orbital energies against eigvalsh(X^T F X) of the
    oracle's matrices, and the levels of each triple equal within themselves."""
    q, m, o, ref = _methane(basis)
    s = q.System(m)
    assert s.n == n
    if basis in GUESS_NOT_UNIQUE:
        # the run starts from the oracle's guess; the product's own guess must be a density of the same kind
        st = q.ScfStepper(s)
        D0, S0 = st.density(0), st.matrix("S")
        st.close()
        assert abs(np.sum(D0 * S0) - 10.0) < 1e-9 and np.abs(D0 @ S0 @ D0 - 2.0 * D0).max() < 1e-9
        st = q.ScfStepper(s, density=o.core_guess()[3])
    else:
        st = q.ScfStepper(s)
    for k in range(len(ref["trace_energy"])):
        e, rms = st.iterate()
        assert abs(e - ref["trace_energy"][k]) < 1e-9 * max(1.0, abs(e)), k
        assert abs(rms - ref["trace_rms"][k]) < 1e-9 + 1e-5 * ref["trace_rms"][k], k
    D, w, S = st.density(0), st.orbital_energies(0), st.matrix("S")
    redos = st.counters()["redos"]
    st.close(); s.close()
    D_ref, w_ref = ref["density"], ref["w_fock"]
    triples, i = [], 0
    while i < n:                                           # levels of the reference: runs of eigenvalues closer than 1e-6
        j = i
        while j + 1 < n and w_ref[j + 1] - w_ref[j] < 1e-6:
            j += 1
        if j - i == 2:
            triples.append((i, j))
        i = j + 1
    spread = max(w[j] - w[i] for i, j in triples)
    print("METHANE %-12s n %2d  passes %2d  redos %g  |dD| %.2e  |tr(DS)-10| %.2e  |dw| %.2e  triples %d  spread %.2e"
          % (basis, n, len(ref["trace_energy"]), redos, np.abs(D - D_ref).max(), abs(np.sum(D * S) - 10.0), np.abs(w - w_ref).max(), len(triples), spread))
    assert np.abs(D - D_ref).max() < 1e-8 * max(1.0, np.abs(D_ref).max())
    assert abs(np.sum(D * S) - 10.0) < 1e-9
    assert np.abs(w - w_ref).max() < 1e-9
    assert (2, 4) in triples and len(triples) >= 2          # the occupied 1t2 level and at least one virtual triple
    assert spread < 1e-9


def test_methane_closed_shell_uhf_reproduces_rhf():
    """UHF (5, 5) on methane/cc-pVDZ: both spins' eigensolves by rotations only, on three-fold degenerate levels"""
    q, m, o, ref = _methane("cc-pVDZ")
    s = q.System(m)
    out = q.unrestricted_hartree_fock(s, q.HartreeFockConfig(100, 1e-10, 5, 5))
    s.close()
    assert out is not None
    print("METHANE uhf cc-pVDZ  dE %.2e  passes %d" % (out.total_energy() - ref["total_energy"], out.iterations))
    assert abs(out.total_energy() - ref["total_energy"]) < TOL_E
