"""GPU parity tests: the HIP path (through the C ABI of libqchem_hip.so) against the CPU oracle on the same inputs.

Tolerances: the path computes in f64; BASELINE.json's north_star asks for total energies within 1e-8 Eh of the CPU
path.  Integrals and Fock matrices are compared element-wise at 1e-10 (abs) - two orders tighter than the energy
target needs - and converged energies at 1e-8 Eh with epsilon = 1e-10 (at looser epsilon the
reference's *reported* energy is itself 6e-8..2e-6 Eh from self-consistency)."""
import os

import numpy as np
import pytest

from conftest import load_system

pytestmark = pytest.mark.gpu

TOL_INT = 1e-10
TOL_E = 1e-8


def _sys(mol, basis):
    import qchem_rs_amd as q
    from oracle.oracle import Oracle
    m = load_system(mol, basis)
    return q, q.System(m), Oracle(m)


def _rand_sym(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    return 0.5 * (A + A.T)


def test_library_is_native_and_device_ready():
    import qchem_rs_amd as q
    assert q.device_ready(), "no gfx950 device: the product path has no CPU fallback"


@pytest.mark.parametrize("mol,basis", [("hydrogen", "STO-3G"), ("water", "STO-3G"), ("water", "6-31G_st_st"),
                                       ("water", "cc-pVDZ"), ("ethylene", "STO-3G"), ("ethylene", "cc-pVDZ"), ("water", "cc-pVTZ")])
def test_eri_tensor_matches_oracle(mol, basis):
    # (ethylene/cc-pVDZ: C spherical d against H p - the shell classes of benzene/cc-pVDZ, BASELINE config 5;
    #  water/cc-pVTZ: the headline configuration - all 11.3 M elements, f shells included)
    q, s, o = _sys(mol, basis)
    I_gpu, I_cpu = s.eri(), o.eri()
    assert np.abs(I_gpu - I_cpu).max() < TOL_INT


def test_eri_tensor_golden_water_sto3g(golden):
    q, s, o = _sys("water", "STO-3G")
    ref = np.array(golden["water/STO-3G"]["eri"]).reshape((7,) * 4)
    assert np.abs(s.eri() - ref).max() < TOL_INT


def test_eri_high_L_blocks_golden(golden):
    """d/f shell quartets of the headline config against the independent numpy vectors (incl. (ff|ff))."""
    q, s, o = _sys("water", "cc-pVTZ")
    I = s.eri()
    g = golden["water/cc-pVTZ"]
    off, L = g["shell_offset"], g["shell_L"]
    nf = lambda l: 2 * l + 1 if l >= 2 else (l + 1) * (l + 2) // 2
    for blk in g["eri_blocks"]:
        sl = tuple(slice(off[i], off[i] + nf(L[i])) for i in blk["shells"])
        ref = np.array(blk["values"]).reshape(blk["shape"])
        assert np.abs(I[sl] - ref).max() < TOL_INT, blk["L"]


@pytest.mark.parametrize("mol,basis", [("water", "STO-3G"), ("water", "cc-pVDZ"), ("water", "cc-pVTZ"),
                                       ("ethylene", "6-31G_st_st"), ("oxygen", "cc-pVDZ")])
def test_fock_rhf_matches_dense_contraction(mol, basis):
    """G from the direct kernels == the reference's dense n^4 contraction (rhf.rs:58-62,152-167) of the oracle's tensor."""
    q, s, o = _sys(mol, basis)
    I = o.eri()
    for seed in (0, 1):
        D = _rand_sym(s.n, seed)
        G_ref = o.g_rhf(D, I)
        G = s.fock_rhf(D)
        scale = max(1.0, np.abs(G_ref).max())
        assert np.abs(G - G_ref).max() < TOL_INT * scale


@pytest.mark.parametrize("mol,basis", [("water", "STO-3G"), ("oxygen", "cc-pVDZ"), ("water", "cc-pVTZ")])
def test_fock_uhf_matches_dense_contraction(mol, basis):
    q, s, o = _sys(mol, basis)
    I = o.eri()
    Da, Db = _rand_sym(s.n, 3), _rand_sym(s.n, 4)
    Ga, Gb = s.fock_uhf(Da, Db)
    Ga_ref, Gb_ref = o.g_uhf(Da, Db, I), o.g_uhf(Db, Da, I)
    scale = max(1.0, np.abs(Ga_ref).max())
    assert np.abs(Ga - Ga_ref).max() < TOL_INT * scale
    assert np.abs(Gb - Gb_ref).max() < TOL_INT * scale


@pytest.mark.parametrize("mol,basis", [("water", "cc-pVDZ"), ("ethylene", "6-31G_st_st"), ("oxygen", "cc-pVDZ"), ("water", "cc-pVTZ")])
def test_pp_ket_bra_major_class_matches_dense_contraction(mol, basis, monkeypatch):
    """The lane-per-quartet kernel for p.p kets (qc_fock_bm_kernel<2, 0>: (pp|pp), (ds|pp)) only takes lists that fill the chip, so the
    small systems of this suite never reach it on their own: QC_BM_PP_MIN = 1 hands it every such quartet.  RHF and UHF digestion against
    the oracle's dense contraction (rhf.rs:152-167, uhf.rs:210-227), and against the column kernels on the same quartets."""
    import qchem_rs_amd as q
    from oracle.oracle import Oracle
    m = load_system(mol, basis)
    o = Oracle(m)
    I = o.eri()
    monkeypatch.setenv("QC_BM_PP_MIN", "1")
    s = q.System(m)
    monkeypatch.delenv("QC_BM_PP_MIN")
    monkeypatch.setenv("QC_NO_BM_PP", "1")
    s_col = q.System(m)
    monkeypatch.delenv("QC_NO_BM_PP")
    names = [u for u in range(q.hf.PROFILE_UNITS) if q.hf.unit_name(u) == "qc_fock_bm_kernel<2, 0>"]
    assert len(names) == 1
    D = _rand_sym(s.n, 5)
    G, G_col, G_ref = s.fock_rhf(D), s_col.fock_rhf(D), o.g_rhf(D, I)
    scale = max(1.0, np.abs(G_ref).max())
    assert np.abs(G - G_ref).max() < TOL_INT * scale
    assert np.abs(G - G_col).max() < 1e-12 * scale
    assert np.array_equal(G, G.T)
    assert np.array_equal(G, s.fock_rhf(D)), "the build is bitwise reproducible with the class switched on"
    Da, Db = _rand_sym(s.n, 6), _rand_sym(s.n, 7)
    Ga, Gb = s.fock_uhf(Da, Db)
    assert np.abs(Ga - o.g_uhf(Da, Db, I)).max() < TOL_INT * scale
    assert np.abs(Gb - o.g_uhf(Db, Da, I)).max() < TOL_INT * scale
    # the class really took quartets (and the column kernels lost exactly those)
    ws, ws_col = s.work_stats(), s_col.work_stats()
    assert ws.quartets == ws_col.quartets
    tp = s.unit_quartets()
    assert tp[names[0]] > 0 and s_col.unit_quartets()[names[0]] == 0
    s.close(); s_col.close()


@pytest.mark.parametrize("mol,basis", [("hydrogen", "STO-3G"), ("water", "6-31G_st_st"), ("water", "cc-pVTZ"), ("oxygen", "cc-pVDZ")])
def test_one_electron_matrices_on_the_gpu(mol, basis):
    """S, T, V from qc_one_electron.hip (what the SCF drivers use) == the oracle's molint::overlap/kinetic/nuclear
    restatement (rhf.rs:41-43), s to f shells, Cartesian and pure."""
    q, s, o = _sys(mol, basis)
    for which, ref in ((0, o.overlap()), (1, o.kinetic()), (2, o.nuclear())):
        M = s.one_electron_gpu(which)
        assert np.abs(M - ref).max() < 1e-11 * max(1.0, np.abs(ref).max())
        assert np.abs(M - M.T).max() == 0.0


def test_cartesian_f_shells_fock_matches_dense_contraction(tmp_path):
    """cc-pVTZ with every d and f shell switched to Cartesian functions (6 and 10 per shell) on O2: the (ff|ff) quartets then
    have 100 x 100 function pairs - more columns than a wave has lanes (several column passes) and more rows than four
    16-row MFMA tiles - paths no shipped basis reaches."""
    import json
    import qchem_rs_amd as q
    from oracle.oracle import Oracle
    from conftest import data
    b = json.load(open(data("basis", "cc-pVTZ.json")))
    for el in b["elements"].values():
        for sh in el["electron_shells"]:
            if sh["angular_momentum"][0] >= 2:
                sh["function_type"] = "gto_cartesian"
    f = tmp_path / "cc-pVTZ-cart.json"
    f.write_text(json.dumps(b))
    m = q.MolecularSystem.load(data("mol", "oxygen.json"), q.BasisSet.load(str(f)))
    s, o = q.System(m), Oracle(m)
    assert s.n == 2 * (4 + 3 * 3 + 2 * 6 + 10)
    I = o.eri()
    D = _rand_sym(s.n, 21)
    G_ref = o.g_rhf(D, I)
    G = s.fock_rhf(D)
    assert np.abs(G - G_ref).max() < TOL_INT * max(1.0, np.abs(G_ref).max())
    for which, ref in ((0, o.overlap()), (1, o.kinetic()), (2, o.nuclear())):
        assert np.abs(s.one_electron_gpu(which) - ref).max() < 1e-11 * max(1.0, np.abs(ref).max())


def test_uhf_spin_square_of_triplet_oxygen():
    """<S^2> from the library == Sz(Sz+1) + N_beta - tr(D_a S D_b S) evaluated with numpy on its densities and the oracle's
    overlap; a triplet UHF determinant is slightly contaminated: a little above 2."""
    q, s, o = _sys("oxygen", "cc-pVDZ")
    st = q.ScfStepper(s, uhf=True, n_alpha=9, n_beta=7)
    for _ in range(25):
        st.iterate()
    Da, Db, S = st.density(0), st.density(1), o.overlap()
    ref = 1.0 * 2.0 + 7 - np.trace(Da @ S @ Db @ S)
    s2 = st.spin_square()
    st.close()
    assert abs(s2 - ref) < 1e-10
    assert 2.0 < s2 < 2.1


def test_fock_without_the_lds_row_buffer(monkeypatch):
    """The bra-major kernels' large-n fallback (exchange contributions as global atomics per bundle, no LDS row buffer)
    gives the same G for both spins' code paths."""
    monkeypatch.setenv("QC_BM_NO_ROWBUF", "1")
    q, s, o = _sys("water", "cc-pVDZ")
    I = o.eri()
    D = _rand_sym(s.n, 11)
    G_ref = o.g_rhf(D, I)
    assert np.abs(s.fock_rhf(D) - G_ref).max() < TOL_INT * max(1.0, np.abs(G_ref).max())
    Da, Db = _rand_sym(s.n, 12), _rand_sym(s.n, 13)
    Ga, Gb = s.fock_uhf(Da, Db)
    Ga_ref, Gb_ref = o.g_uhf(Da, Db, I), o.g_uhf(Db, Da, I)
    assert np.abs(Ga - Ga_ref).max() < TOL_INT * max(1.0, np.abs(Ga_ref).max())
    assert np.abs(Gb - Gb_ref).max() < TOL_INT * max(1.0, np.abs(Gb_ref).max())


def test_fock_linearity_and_symmetry_benzene_ccpvdz():
    """Full-size property test (BASELINE config 5, n = 114): G is linear in D and symmetric."""
    q, s, o = _sys("benzene", "cc-pVDZ")
    D1, D2 = _rand_sym(s.n, 5), _rand_sym(s.n, 6)
    G1, G2, G12 = s.fock_rhf(D1), s.fock_rhf(D2), s.fock_rhf(D1 + 2.0 * D2)
    scale = np.abs(G12).max()
    assert np.abs(G12 - (G1 + 2.0 * G2)).max() < 1e-11 * scale
    assert np.abs(G1 - G1.T).max() < 1e-11 * scale


def test_fock_benzene_equals_contraction_of_the_materialised_tensor():
    """Full size (BASELINE config 5, 1.1 M quartets): the fused digestion (row buffers, MFMA step 3, atomics, replicas) against
    a plain numpy contraction of the tensor the same integral code materialises (qc_eri_full; that tensor is pinned against the
    oracle element by element at this size in test_eri_tensor_above_n64_matches_oracle)."""
    q, s, o = _sys("benzene", "cc-pVDZ")
    n = s.n
    I = s.eri()
    D = _rand_sym(n, 31)
    J = np.tensordot(I.reshape(n * n, n * n), D.reshape(-1), axes=([1], [0])).reshape(n, n)
    K = np.einsum("ikjl,kl->ij", I, D, optimize=True)
    G_ref = J - 0.5 * K
    G = s.fock_rhf(D)
    assert np.abs(G - G_ref).max() < 1e-11 * max(1.0, np.abs(G_ref).max())


def test_sharded_fock_sums_to_full():
    q, s, o = _sys("water", "cc-pVDZ")
    D = _rand_sym(s.n, 7)
    G_full = s.fock_rhf(D)
    acc = np.zeros_like(G_full)
    for r in range(3):
        s.set_shard(r, 3)
        acc += s.fock_rhf(D)
    s.set_shard(0, 1)
    assert np.abs(acc - G_full).max() < 1e-11 * np.abs(G_full).max()


def test_rccl_path_single_rank_communicator():
    """The multi-GPU build path (shard + RCCL all-reduce of the partial Fock matrix) with a 1-rank communicator:
    exercises ncclGetUniqueId / ncclCommInitRank / ncclAllReduce inside libqchem_hip.so on real hardware."""
    q, s, o = _sys("water", "STO-3G")
    s.comm_init(q.comm_unique_id(), 0, 1)
    D = _rand_sym(s.n, 9)
    assert np.abs(s.fock_rhf(D) - o.g_rhf(D, o.eri())).max() < TOL_INT * 10
    Ga, Gb = s.fock_uhf(D, 0.5 * D)
    assert np.abs(Ga - o.g_uhf(D, 0.5 * D, o.eri())).max() < TOL_INT * 10
    # the whole multi-rank SCF pass (integer all-reduce of the hi / lo planes, pass scalars all-reduced as bit patterns and
    # checked for agreement before any decision is taken) with that communicator: same result as without one, bit for bit
    out = q.restricted_hartree_fock(s, q.HartreeFockConfig(100, 1e-10))
    ref = o.rhf(100, 1e-10)
    assert out is not None and abs(out.total_energy() - ref["total_energy"]) < TOL_E and out.iterations == ref["iterations"]
    s1 = q.System(load_system("water", "STO-3G"))
    out1 = q.restricted_hartree_fock(s1, q.HartreeFockConfig(100, 1e-10))
    assert out1.electronic_energy == out.electronic_energy and out1.orbital_energies == out.orbital_energies
    outu = q.unrestricted_hartree_fock(s, q.HartreeFockConfig(100, 1e-10))
    assert outu is not None and abs(outu.total_energy() - ref["total_energy"]) < TOL_E
    assert "rccl" in q.rccl_info().lower()


def test_repeat_branch_with_a_communicator(monkeypatch):
    """The repeat branch of a pass (scf_iterate: a refinement that asks for rotations -> the eigensolve again, new density, the scalars
    published a second time - the one place where a multi-rank pass issues a second collective) with a 1-rank communicator.  Reached on
    purpose: QC_EIG_WARM_RMS = 0.5 lets the perturbative refinement start while the density still moves by 0.1 per element.  The
    trajectory may differ from the default path in its last bits (other eigensolver per pass), the fixed point may not."""
    import qchem_rs_amd as q
    m = load_system("ethylene", "cc-pVDZ")                 # n = 48: one-workgroup path without a communicator, generic path with one
    s0 = q.System(m)
    e0 = q.restricted_hartree_fock(s0, q.HartreeFockConfig(100, 1e-10))
    monkeypatch.setenv("QC_EIG_WARM_RMS", "0.5")
    for comm in (False, True):
        s = q.System(m)
        if comm:
            s.comm_init(q.comm_unique_id(), 0, 1)
        st = q.ScfStepper(s)
        e = r = None
        for k in range(60):
            e, r = st.iterate()
            if r < 1e-10:
                break
        c = st.counters()
        st.close(); s.close()
        assert r < 1e-10 and c["redos"] >= 1, (comm, c)
        assert abs(e - e0.electronic_energy) < 1e-9, (comm, e, e0.electronic_energy)
    s0.close()


def test_step_api_matches_driver():
    """qc_scf_begin/iterate/end (the entry points a host-owned convergence loop binds) == qc_scf_rhf."""
    q, s, o = _sys("water", "cc-pVDZ")
    st = q.ScfStepper(s)
    e = rms = None
    for it in range(100):
        e, rms = st.iterate()
        if rms < 1e-10:
            break
    out = q.restricted_hartree_fock(s, q.HartreeFockConfig(100, 1e-10))
    assert out.iterations == it and abs(e - out.electronic_energy) < 1e-9
    assert np.abs(st.orbital_energies() - np.array(out.orbital_energies)).max() < 1e-9
    st.close()


@pytest.mark.parametrize("n", [2, 7, 24, 58, 64, 65, 114, 128, 129, 150, 174, 192, 193, 230])
def test_sym_eig(n):
    """utils.rs:15-36 through qc_sym_eig.  The sizes sit on both sides of every kernel switch of the cold path: rotations below 24, the
    register Householder kernels for n <= 64 / 128 / 192, the LDS- or memory-resident one above; back-transformation in one or several
    LDS chunks of reflector rows."""
    import qchem_rs_amd as q
    s = q.System(load_system("hydrogen", "STO-3G"))
    A = _rand_sym(n, n)
    V, w = s.sym_eig(A)
    w_ref = np.linalg.eigvalsh(A)
    assert np.all(np.diff(w) >= 0)
    assert np.abs(w - w_ref).max() < 1e-12 * max(1.0, np.abs(w_ref).max())
    assert np.abs(V.T @ V - np.eye(n)).max() < 1e-12
    assert np.abs(A @ V - V * w).max() < 1e-11 * max(1.0, np.abs(w_ref).max())


def test_sym_eig_warm_start_regimes():
    """qc_sym_eig_warm: GEMM refinement for small perturbations, Jacobi fallback for large ones, (near-)degenerate spectra."""
    import qchem_rs_amd as q
    s = q.System(load_system("hydrogen", "STO-3G"))
    rng = np.random.default_rng(2)
    n = 40
    for split in (0.0, 1e-9, 1e-5):
        d = np.sort(rng.uniform(-10, 10, n)); d[1] = d[0] + split; d[11] = d[10] + split; d[21] = d[20] + split; d[22] = d[20] + 2 * split
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        A = (Q * d) @ Q.T; A = 0.5 * (A + A.T)
        _, V0 = np.linalg.eigh(A)
        for eps in (0.0, 1e-9, 1e-6, 1e-3, 0.3):
            P = rng.standard_normal((n, n)); B = A + eps * (P + P.T)
            V, w = s.sym_eig_warm(B, V0)
            assert np.all(np.diff(w) >= 0)
            assert np.abs(w - np.linalg.eigvalsh(B)).max() < 1e-11
            assert np.abs(V.T @ V - np.eye(n)).max() < 1e-12
            assert np.abs(B @ V - V * w).max() < 1e-10


def test_rhf_chloroform_sto3g_third_row_and_large_basis():
    """Cl (6-primitive contractions, 33 functions) and a basis beyond the in-LDS eigensolver limit (benzene/6-311++G**, n = 174).
    The G(2D) = 2 G(D) line holds by construction under fixed-point accumulation (the scale drops by one, every contribution doubles
    exactly): it is no parity check - test_fock_above_n64_matches_the_oracle_quartet_contraction compares that build with the oracle."""
    q, s, o = _sys("chloroform", "STO-3G")
    out = q.restricted_hartree_fock(s, q.HartreeFockConfig(200, 1e-9))
    ref = o.rhf(200, 1e-9)
    assert out is not None and ref["status"] == 0 and abs(out.total_energy() - ref["total_energy"]) < TOL_E
    q, s, o = _sys("benzene", "6-311++G_st_st")
    assert s.n > 128
    D = _rand_sym(s.n, 12)
    G1, G2 = s.fock_rhf(D), s.fock_rhf(2.0 * D)
    assert np.abs(G2 - 2.0 * G1).max() < 1e-10 * np.abs(G2).max()
    st = q.ScfStepper(s)
    e0, r0 = st.iterate()
    e1, r1 = st.iterate()
    assert np.isfinite(e0) and np.isfinite(e1) and r1 < r0
    st.close()


def test_sym_eig_degenerate():
    import qchem_rs_amd as q
    s = q.System(load_system("hydrogen", "STO-3G"))
    rng = np.random.default_rng(0)
    Q, _ = np.linalg.qr(rng.standard_normal((12, 12)))
    w0 = np.array([-2.0, -2.0, -2.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 3.0, 5.0, 5.0])
    A = (Q * w0) @ Q.T
    V, w = s.sym_eig(0.5 * (A + A.T))
    assert np.abs(w - np.sort(w0)).max() < 1e-12
    assert np.abs(V.T @ V - np.eye(12)).max() < 1e-12


@pytest.mark.parametrize("mol,basis", [("hydrogen", "STO-3G"), ("water", "STO-3G"), ("water", "cc-pVDZ"),
                                       ("water", "cc-pVTZ"), ("ethylene", "STO-3G")])
def test_rhf_energy_matches_oracle(mol, basis):
    q, s, o = _sys(mol, basis)
    cfg = q.HartreeFockConfig(max_iterations=100, epsilon=1e-10)
    out = q.restricted_hartree_fock(s, cfg)
    ref = o.rhf(100, 1e-10)
    assert out is not None and ref["status"] == 0
    assert abs(out.total_energy() - ref["total_energy"]) < TOL_E
    assert abs(out.nuclear_repulsion - ref["nuclear_repulsion"]) < 1e-12
    assert np.abs(np.array(out.orbital_energies) - ref["orbital_energies"]).max() < 1e-7


def test_rhf_literature_energies():
    """Literature pins reproduced on the GPU: PySCF-documented H2O/cc-pVDZ, Szabo-Ostlund H2/STO-3G, H2O/cc-pVTZ to the four
    published decimals and the hydrogen atom in cc-pVTZ (one-electron matrices from qc_one_electron.hip)."""
    q, s, o = _sys("water_eq", "cc-pVDZ")
    out = q.restricted_hartree_fock(s, q.HartreeFockConfig(100, 1e-10))
    assert abs(out.total_energy() - (-76.0267656731)) < 2e-9
    q, s, o = _sys("hydrogen", "STO-3G")
    out = q.restricted_hartree_fock(s, q.HartreeFockConfig(100, 1e-12))
    assert abs(out.total_energy() - (-1.1167)) < 5e-5
    # the headline basis (tests/test_oracle_known_answers.py has the provenance of both numbers)
    q, s, o = _sys("water_eq", "cc-pVTZ")
    out = q.restricted_hartree_fock(s, q.HartreeFockConfig(100, 1e-10))
    assert abs(out.total_energy() - (-76.0571)) < 1.5e-4
    import scipy.linalg as sl
    q, s, o = _sys("h_atom", "cc-pVTZ")
    w = sl.eigh(s.one_electron_gpu(1) + s.one_electron_gpu(2), s.one_electron_gpu(0), eigvals_only=True)
    assert abs(w[0] - (-0.49980981)) < 1e-8


@pytest.mark.parametrize("mol,basis", [("water", "STO-3G"), ("oxygen", "cc-pVDZ")])
def test_uhf_reference_rule_matches_oracle(mol, basis):
    """uhf.rs:43-45: n_alpha = n_beta = N/2 - the only open-shell behaviour the reference has."""
    q, s, o = _sys(mol, basis)
    out = q.unrestricted_hartree_fock(s, q.HartreeFockConfig(100, 1e-10))
    ref = o.uhf(100, 1e-10)
    assert out is not None and ref["status"] == 0
    assert abs(out.total_energy() - ref["total_energy"]) < TOL_E


def test_uhf_triplet_oxygen_extension():
    """BASELINE config 4: O2 triplet (n_alpha = 9, n_beta = 7) - an extension, checked against the oracle's same extension.

    The symmetric determinant the reference algorithm settles on is a saddle of the UHF functional (a symmetry-broken one
    lies 0.024 Eh lower) and the never-reset DIIS(2,8) of uhf.rs:76-78 crawls on it at a density rms of 1e-9..1e-10.  The
    iteration stays there as long as nothing seeds the unstable direction: the reference's fixed sequence of operations
    does not, and neither does the fixed-point accumulation of the GPU build (f64 atomics did, in one run of five).  One
    outcome, asserted three ways."""
    q, s, o = _sys("oxygen", "cc-pVDZ")
    ref = o.uhf(2000, 1e-10, n_alpha=9, n_beta=7)
    assert ref["status"] == 0

    def run():
        st = q.ScfStepper(s, uhf=True, n_alpha=9, n_beta=7)
        trace = []
        for _ in range(2001):
            e, rms = st.iterate()
            trace.append((e, rms))
            if rms / 2.0 < 1e-10:                              # uhf.rs:139
                break
        Da, Db = st.density(0), st.density(1)
        st.close()
        return trace, Da, Db

    trace, Da, Db = run()
    e, rms = trace[-1]
    assert rms / 2.0 < 1e-10
    # (1) the variational energy of the converged densities, evaluated by the oracle for both sides
    I, H = o.eri(), o.kinetic() + o.nuclear()
    evar = lambda A, B: 0.5 * np.sum(A * (2 * H + o.g_uhf(A, B, I))) + 0.5 * np.sum(B * (2 * H + o.g_uhf(B, A, I)))
    assert abs(evar(Da, Db) - evar(ref["density_alpha"], ref["density_beta"])) < 1e-9
    # (2) the energy as the reference reports it (stale G, uhf.rs:145-153) within the north-star bar
    assert abs(e + s.nuclear_repulsion() - ref["total_energy"]) < TOL_E
    # (3) a second run repeats the first bit for bit - every pass's energy and rms
    trace2, Da2, Db2 = run()
    assert trace2 == trace and np.array_equal(Da2, Da) and np.array_equal(Db2, Db)


def test_fock_build_is_bitwise_reproducible():
    """Fixed-point accumulation (default): a build does not depend on the order the GPU serves its atomic adds in - same
    bits from repeated builds, from a fresh handle (its own stream tuning) and for the two spins of a closed-shell UHF
    build (the reference's identical per-spin arithmetic, uhf.rs:80-108, 210-227).  The f64-atomic mode agrees to rounding."""
    q, s, o = _sys("water", "cc-pVTZ")
    D = _rand_sym(s.n, 41)
    G0 = s.fock_rhf(D)
    assert np.array_equal(G0, G0.T)
    for _ in range(3):
        assert np.array_equal(s.fock_rhf(D), G0)
    s2 = q.System(load_system("water", "cc-pVTZ"))
    assert np.array_equal(s2.fock_rhf(D), G0)
    Ga, Gb = s.fock_uhf(D, D)
    assert np.array_equal(Ga, Gb)
    I = o.eri()
    assert np.abs(Ga - o.g_uhf(D, D, I)).max() < TOL_INT * max(1.0, np.abs(Ga).max())
    # partial matrices of a sharded build are integers too: their sum is the full matrix
    acc = np.zeros_like(G0)
    for r in range(4):
        s2.set_shard(r, 4)
        acc += s2.fock_rhf(D)
    assert np.abs(acc - G0).max() < 1e-13 * np.abs(G0).max()
    s2.set_accumulation("f64")
    s2.set_shard(0, 1)
    assert np.abs(s2.fock_rhf(D) - G0).max() < 1e-12 * np.abs(G0).max()
    s2.close()


def test_launch_structure_switches_do_not_change_a_bit(monkeypatch):
    """How a build's launches are issued and joined is not allowed to show in the result (integer accumulation): the device-side join
    of the side streams against the event join it replaced (QC_EVENT_JOIN - also what a handle falls back to when dispatches are
    serialised, e.g. under rocprofv3 --pmc), and the end of an SCF pass seen through the pinned sequence word against the stream's
    event (QC_EVENT_WAIT).  The switches are read per handle / per SCF state."""
    import qchem_rs_amd as q
    m = load_system("water", "cc-pVTZ")
    D = _rand_sym(58, 43)
    s0 = q.System(m)
    G0 = s0.fock_rhf(D)
    e0 = q.restricted_hartree_fock(s0, q.HartreeFockConfig(100, 1e-10))
    # (QC_NO_LANES: launch units drawn among all seven side streams instead of the four dispatch lanes)
    # (QC_NO_BM_MERGE / QC_NO_T1_MERGE: the merged launches of the small builds apart again - 9 and 11 launches instead of 8; QC_NREP_USE: all
    # 32 accumulator replicas instead of 8)
    for env in ({"QC_EVENT_JOIN": "1"}, {"QC_EVENT_WAIT": "1"}, {"QC_NO_LANES": "1"}, {"QC_NO_BM_MERGE": "1"}, {"QC_NO_T1_MERGE": "1"},
                {"QC_NO_BM_MERGE": "1", "QC_NO_T1_MERGE": "1", "QC_NREP_USE": "32"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        s = q.System(m)
        for _ in range(3):
            assert np.array_equal(s.fock_rhf(D), G0), env
        Ga, Gb = s.fock_uhf(D, D)
        assert np.array_equal(Ga, Gb)
        e = q.restricted_hartree_fock(s, q.HartreeFockConfig(100, 1e-10))
        assert e.iterations == e0.iterations and e.electronic_energy == e0.electronic_energy and e.orbital_energies == e0.orbital_energies, env
        s.close()
        for k in env:
            monkeypatch.delenv(k)
    s0.close()


@pytest.mark.parametrize("mol,basis,uhf,na,nb,EPS", [("water", "cc-pVTZ", False, 0, 0, 1e-9), ("water", "cc-pVDZ", True, 0, 0, 1e-9), ("oxygen", "cc-pVDZ", True, 9, 7, 1e-9),
                                                     ("ethylene", "cc-pVDZ", False, 0, 0, 1e-9), ("benzene", "6-31G_st_st", False, 0, 0, 1e-6)])
def test_stepper_and_driver_agree_with_and_without_a_stop_rule(mol, basis, uhf, na, nb, EPS):
    """Announcing the host's stopping rule (qc_scf_set_stop_rule) changes nothing: a stepper without a rule and one with it, both stepped
    two passes beyond convergence, give the same passes bit for bit; a second run on the same handle (tuned streams) reproduces the first;
    the whole-run driver on that handle stops at the same pass with the same energy; the reserved counters stay 0.  All launch paths:
    one-workgroup RHF, closed-shell UHF on that path, open-shell and n > 64 (generic sequence, event wait)."""
    import qchem_rs_amd as q
    m = load_system(mol, basis)

    def run(stop_rule, extra, s):
        st = q.ScfStepper(s, uhf=uhf, n_alpha=na, n_beta=nb, stop_rule=stop_rule)
        tr, k_conv = [], None
        for k in range(60):
            e, r = st.iterate()
            tr.append((e, r))
            if k_conv is None and (r / 2 if uhf else r) < EPS:
                k_conv = k
            if k_conv is not None and k >= k_conv + extra:
                break
        c = st.counters()
        st.close()
        return tr, k_conv, c

    s_ref = q.System(m)
    ref, k_ref, c_ref = run(0.0, 2, s_ref)
    assert k_ref is not None and c_ref["spec_hits"] == 0 and c_ref["spec_lost"] == 0
    s = q.System(m)
    warm, _, c_w = run(0.0, 0, s)                                 # (first run on a handle: its first build tunes the streams)
    assert warm == ref[:len(warm)]
    a, k_a, c_a = run(0.0, 2, s)                                  # no rule announced
    assert a == ref and k_a == k_ref
    b, k_b, c_b = run(EPS, 2, s)                                  # rule announced, host goes on for two more passes anyway
    assert b == ref and k_b == k_ref
    for c in (c_w, c_a, c_b):
        assert c["spec_hits"] == 0 and c["spec_lost"] == 0, c
    out = (q.unrestricted_hartree_fock if uhf else q.restricted_hartree_fock)(s, q.HartreeFockConfig(100, EPS, na, nb))
    assert out.iterations == k_ref and out.electronic_energy == ref[k_ref][0]
    s.close(); s_ref.close()


def test_a_wait_that_gives_up_fails_the_call_that_waited(monkeypatch):
    """A device-side wait (the join of a build's side streams) that runs into its limit has folded an incomplete
    matrix: the call whose host wait follows it returns QC_ERR_HIP (never a wrong G), and the handle goes on with event joins.  Forced
    here: QC_JOIN_FAULT leaves one side stream's marker out (a join that can never complete, as if a launch had died) and the limit is
    2 ms (QC_WAIT_LIMIT_MS)."""
    import qchem_rs_amd as q
    m = load_system("water", "cc-pVTZ")
    D = _rand_sym(58, 7)
    s = q.System(m)
    G0 = s.fock_rhf(D)                                            # device join, nothing wrong
    s2 = q.System(m)
    G2 = s2.fock_rhf(D)                                           # (its first build: launches timed alone, lanes, proposals)
    assert np.array_equal(G2, G0)
    monkeypatch.setenv("QC_WAIT_LIMIT_MS", "2")
    monkeypatch.setenv("QC_JOIN_FAULT", "1")
    with pytest.raises(q.hf.QcError):
        s2.fock_rhf(D)                                            # THIS call fails: its join gave up
    st = q.ScfStepper(s)                                          # ... and so does the SCF pass whose build's join gives up
    with pytest.raises(q.hf.QcError):
        for _ in range(3):
            st.iterate()
    st.close()
    monkeypatch.delenv("QC_JOIN_FAULT")
    monkeypatch.delenv("QC_WAIT_LIMIT_MS")
    for h in (s, s2):                                             # event joins from now on: complete results again
        assert np.array_equal(h.fock_rhf(D), G0)
    out = q.restricted_hartree_fock(s2, q.HartreeFockConfig(100, 1e-10))
    ref = q.restricted_hartree_fock(q.System(m), q.HartreeFockConfig(100, 1e-10))
    assert out.iterations == ref.iterations and out.electronic_energy == ref.electronic_energy
    s.close(); s2.close()


def test_two_handles_from_two_threads():
    """`distinct handles may be used from distinct threads` (include/qchem_hip.h): two SCF runs on one device at the same time - both
    with device-side waits - end bit-identical to the same runs alone (per-device issue gate, qc_streams.hip)."""
    import threading
    import qchem_rs_amd as q
    mols = [load_system("water", "cc-pVTZ"), load_system("ethylene", "cc-pVDZ")]
    cfg = q.HartreeFockConfig(100, 1e-10)
    alone = []
    hs = [q.System(m) for m in mols]
    for h in hs:
        alone.append(q.restricted_hartree_fock(h, cfg))
    res = [[None] * 3, [None] * 3]

    def work(i):
        for r in range(3):
            res[i][r] = q.restricted_hartree_fock(hs[i], cfg)

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in th)
    for i in range(2):
        for r in range(3):
            o = res[i][r]
            assert o is not None and o.iterations == alone[i].iterations and o.electronic_energy == alone[i].electronic_energy
            assert o.orbital_energies == alone[i].orbital_energies
    # one thread stepping two states of two handles alternately (the waits of one are in flight while the other issues)
    st = [q.ScfStepper(h, stop_rule=1e-10) for h in hs]
    tr = [[], []]
    for k in range(12):
        for i in range(2):
            tr[i].append(st[i].iterate())
    for i in range(2):
        st[i].close()
        one = q.ScfStepper(hs[i]); ref = [one.iterate() for _ in range(12)]; one.close()
        assert tr[i] == ref
    for h in hs:
        h.close()


@pytest.mark.parametrize("mol,basis,na,nb", [("oxygen", "cc-pVDZ", 9, 7), ("water", "cc-pVDZ", 0, 0), ("benzene", "6-31G_st_st", 0, 0)])
def test_spin_parallel_roothaan_steps_do_not_change_a_bit(mol, basis, na, nb, monkeypatch):
    """UHF passes on the generic launch sequence run the alpha and the beta Roothaan step side by side on two streams (scf_iterate).  Same
    kernels and arithmetic per spin: every pass - energy, rms, and at the end the orbital energies - is bit for bit the serial order's
    (QC_NO_SPIN_PARALLEL), also for the O2 triplet, whose trajectory forgives nothing."""
    import qchem_rs_amd as q
    m = load_system(mol, basis)

    def run():
        s = q.System(m)
        st = q.ScfStepper(s, uhf=True, n_alpha=na, n_beta=nb)
        tr = [st.iterate() for _ in range(30)]
        w = (st.orbital_energies(0), st.orbital_energies(1))
        st.close(); s.close()
        return tr, w

    par, wp = run()
    monkeypatch.setenv("QC_NO_SPIN_PARALLEL", "1")
    ser, ws = run()
    assert par == ser
    assert np.array_equal(wp[0], ws[0]) and np.array_equal(wp[1], ws[1])


def test_assignment_search_and_replica_count_never_show(monkeypatch):
    """Which launch goes to which dispatch lane is searched while the handle is used (qc_assign.hip: trials of neighbouring assignments,
    restarts from perturbed copies of the best, finals) and how many accumulator replicas are in use is a tuning matter (8 for n <= 64):
    neither may change a bit of any build or of any SCF run - and the search ends, by itself or when a harness says so."""
    import qchem_rs_amd as q
    m = load_system("water", "cc-pVTZ")
    D = _rand_sym(58, 47)
    monkeypatch.setenv("QC_NO_ASSIGN_CACHE", "1")              # (a fresh search, whatever this process has learned before)
    s = q.System(m)
    G0 = s.fock_rhf(D)
    first, trials = None, 0.0
    for run in range(14):
        st = q.ScfStepper(s, stop_rule=1e-10)
        es = []
        for k in range(40):
            e, rms = st.iterate()
            es.append(e)
            if rms < 1e-10:
                break
        c = st.counters()
        st.close()
        trials = max(trials, c["assign_trials"])
        if first is None:
            first = es
        assert es == first, run                                  # every pass of every run: the same bits, whatever was being tried
    assert trials > 0                                            # (the search did run inside these SCF runs)
    assert np.array_equal(s.fock_rhf(D), G0)
    s.freeze_assignment()
    st = q.ScfStepper(s, stop_rule=1e-10)
    st.iterate()
    assert st.counters()["assign_frozen"] > 0
    st.close()
    s.close()
    for nrep in ("32", "3"):                                     # integer sums do not depend on how they are split over replicas
        monkeypatch.setenv("QC_NREP_USE", nrep)
        s2 = q.System(m)
        assert np.array_equal(s2.fock_rhf(D), G0), nrep
        s2.close()
        monkeypatch.delenv("QC_NREP_USE")


def test_device_timeline_and_host_stamps(monkeypatch, capfd):
    """QC_DEV_TIMELINE / QC_ISSUE_DEBUG (diagnostics): every kernel of an SCF pass leaves its start and end on the device's
    constant clock, the host its time stamps between the end of a pass and the launches of the next - printed when the SCF state ends /
    after every pass, and switched on per pass."""
    q, s, o = _sys("water", "cc-pVDZ")
    st = q.ScfStepper(s)
    st.iterate()                                                 # (not traced)
    monkeypatch.setenv("QC_DEV_TIMELINE", "1")
    for _ in range(3):
        st.iterate()
    monkeypatch.delenv("QC_DEV_TIMELINE")
    e_traced, _ = st.iterate()
    st.close()
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("[timeline] pass")]
    assert len(lines) == 3, err
    for l in lines:
        assert " fold " in l and " small " in l and " unit" in l, l
        import re
        spans = re.findall(r"(\w+) (\d+\.\d+)-(\d+\.\d+)", l)
        assert len(spans) >= 3 and all(float(b) >= float(a) for _, a, b in spans), l
    # the diagnostics do not touch the arithmetic
    st2 = q.ScfStepper(s)
    for _ in range(4):
        st2.iterate()
    e_plain, _ = st2.iterate()
    st2.close()
    assert e_plain == e_traced


def test_ds_lane_order_is_probed_and_a_device_that_fails_loses_nothing_but_time(monkeypatch):
    """The exchange rows of a bra-major bundle are pre-summed with f64 DS atomics, several lanes of one instruction adding to one word: bitwise
    reproducibility needs the DS unit to serve them in a fixed order.  qc_ds_order_probe asks the device at set-up (64 x the same 64-lane add
    with values of very different magnitudes: all sums the same bits); a device that failed would get the direct fixed-point global atomics -
    here forced (QC_DS_ORDER_FAIL): same matrix to rounding, still reproducible bit for bit, still symmetric."""
    import qchem_rs_amd as q
    m = load_system("benzene", "6-31G_st_st")
    s = q.System(m)
    D = _rand_sym(s.n, 53)
    G = s.fock_rhf(D)
    s.close()
    monkeypatch.setenv("QC_DS_ORDER_FAIL", "1")
    s2 = q.System(m)
    G2 = s2.fock_rhf(D)
    assert np.array_equal(G2, s2.fock_rhf(D)) and np.array_equal(G2, G2.T)
    assert np.abs(G2 - G).max() < 1e-12 * max(1.0, np.abs(G).max())
    s2.close()


def test_dispatch_lanes_are_measured():
    """qc_lane_probe: the handle's side streams fall into dispatch lanes (streams that share a pipe wait for each other's grids); the
    assignment slots list every side stream once, the lanes first.  On an MI355X with GPU_MAX_HW_QUEUES=8 (set by hf.py) there are four."""
    q, s, o = _sys("water", "STO-3G")
    n, slots, lane0_main = s.dispatch_lanes()
    assert sorted(slots) == list(range(7))
    assert 1 <= n <= 7
    if os.environ.get("GPU_MAX_HW_QUEUES") == "8" and not os.environ.get("QC_NO_LANES"):
        assert n == 4 and lane0_main, (n, slots, lane0_main)


def test_handle_lifecycle():
    """What the device side of a handle goes through from its creation to its end (qc_device.cpp, the stream pool of qc_streams.hip,
    qc_system_destroy): a handle that closes leaves its stream set to the next one, which reports the same dispatch lanes and builds the
    same bits; a handle closed under a live SCF state stays until that state ends, and the state's passes are those of an undisturbed run;
    the device is in order afterwards.  water/6-31G** (n = 25): a bra-major and a column class in one build."""
    import qchem_rs_amd as q
    m = load_system("water", "6-31G_st_st")
    D = _rand_sym(25, 11)
    s1 = q.System(m)
    G = s1.fock_rhf(D)
    lanes = s1.dispatch_lanes()
    s1.close()
    s2 = q.System(m)
    if not os.environ.get("QC_NO_LANES") and not os.environ.get("QC_NO_STREAM_POOL"):
        assert s2.dispatch_lanes() == lanes                        # (the pooled stream set came back with its measured lanes)
    assert np.array_equal(s2.fock_rhf(D), G)
    s2.close()

    def passes(close_handle_after):
        h = q.System(m)
        st = q.ScfStepper(h)
        tr = []
        for k in range(5):
            if k == close_handle_after:
                h.close()                                          # the state keeps the handle alive
            tr.append(st.iterate())
        w = st.orbital_energies()
        st.close()                                                 # (the last state of a closed handle frees it)
        h.close()
        return tr, w

    ref, w_ref = passes(None)
    tr, w = passes(2)
    assert tr == ref and np.array_equal(w, w_ref)
    s4 = q.System(m)
    assert np.array_equal(s4.fock_rhf(D), G)
    s4.close()


def test_scf_runs_are_bitwise_reproducible():
    q, s, o = _sys("water", "cc-pVDZ")
    outs = [q.restricted_hartree_fock(s, q.HartreeFockConfig(100, 1e-10)) for _ in range(2)]
    assert outs[0].iterations == outs[1].iterations and outs[0].electronic_energy == outs[1].electronic_energy
    assert outs[0].orbital_energies == outs[1].orbital_energies


def test_schwarz_factors_and_screening():
    """Schwarz pass: the screened build (default tau = 1e-12) against the unscreened one and the oracle; the count of
    surviving quartets is reported, never more than enumerated; tau = 0 restores every quartet."""
    q, s, o = _sys("ethylene", "6-31G_st_st")
    D = _rand_sym(s.n, 51)
    G = s.fock_rhf(D)                                   # device pass has run: lists are screened
    ws = s.work_stats()
    assert ws.schwarz_tau == 1e-12 and ws.quartets_enumerated == s.n_quartets()
    assert 0 <= ws.quartets_screened_out < ws.quartets_enumerated and ws.quartets + ws.quartets_screened_out <= ws.quartets_enumerated
    G_ref = o.g_rhf(D, o.eri())
    assert np.abs(G - G_ref).max() < TOL_INT * max(1.0, np.abs(G_ref).max())
    s.set_schwarz(0.0)
    ws0 = s.work_stats()
    assert ws0.quartets_screened_out == 0 and ws0.quartets >= ws.quartets
    G_all = s.fock_rhf(D)
    assert np.abs(G_all - G).max() < TOL_INT * max(1.0, np.abs(G_ref).max())


@pytest.mark.parametrize("mol,basis,na,nb", [("water", "cc-pVDZ", 0, 0), ("oxygen", "cc-pVDZ", 9, 7), ("water", "cc-pVTZ", 0, 0), ("ethylene", "6-31G_st_st", 0, 0),
                                             ("ethylene", "cc-pVTZ", 0, 0)])
def test_uhf_passes_match_oracle_one_by_one(mol, basis, na, nb):
    """The UHF loop body (uhf.rs:80-163) pass by pass: both Fock matrices from the OLD densities, per-spin DIIS(2,8), the averaged
    rms of uhf.rs:137 and the energy expression of uhf.rs:145-153 - closed shell under the reference's N/2 rule, and the open-shell
    extension while its trajectory is still well conditioned (the first passes; later it amplifies rounding, see the triplet test).
    (ethylene/cc-pVTZ, n = 116: the generic launch sequence with f functions and the one-sided rotation kernel in LDS.)"""
    q, s, o = _sys(mol, basis)
    npass = 12 if na else 100
    I, _ = o.eri_strided_mt(0, 1, min(16, len(os.sched_getaffinity(0))))
    ref = o.uhf(npass if na else 100, 1e-10 if not na else 1e-30, n_alpha=na or -1, n_beta=nb or -1, eri=I, trace=True)
    del I
    st = q.ScfStepper(s, uhf=True, n_alpha=na, n_beta=nb)
    for k in range(min(len(ref["trace_energy"]), npass if na else 1000)):
        e, rms = st.iterate()
        tol = 1e-9 if not na else 1e-7          # (the triplet's differences grow about tenfold per pass from 1e-12)
        assert abs(e - ref["trace_energy"][k]) < tol * max(1.0, abs(e)), k
        assert abs(rms - ref["trace_rms"][k]) < tol + 1e-4 * ref["trace_rms"][k], k
    st.close()


def test_benzene_ccpvdz_fock_against_the_oracle_on_a_shard():
    """BASELINE config 5 at full size against the oracle: one shard of eight of the product's own work plan (~135 k shell
    quartets over every class of benzene/cc-pVDZ) digested by the GPU and by the oracle's quartet-list contraction
    (orc_g_rhf_quartets: the reference's (ij|kl) D_kl - 1/2 (ik|jl) D_kl sums, rhf.rs:58-62,152-167, restricted to the list)."""
    q, s, o = _sys("benzene", "cc-pVDZ")
    D = _rand_sym(s.n, 61)
    G_full = s.fock_rhf(D)                              # (initialises the device: Schwarz factors, screened lists)
    s.set_shard(3, 8)
    abcd = s.plan_shard_quartets(3, 8)
    assert 100_000 < len(abcd) < 160_000
    G = s.fock_rhf(D)
    G_ref = o.g_rhf_quartets(D, abcd)
    scale = max(1.0, np.abs(G_full).max())
    assert np.abs(G - G_ref).max() < TOL_INT * scale
    # the screened-out quartets are below the parity bar as a whole: unscreened full build == screened full build
    s.set_shard(0, 1)
    s.set_schwarz(0.0)
    assert np.abs(s.fock_rhf(D) - G_full).max() < TOL_INT * scale


def test_benzene_ccpvdz_energy_matches_oracle():
    """BASELINE config 5, converged energy.  The oracle stalls at a density rms of ~3e-9 (near-degenerate orbitals, never-reset DIIS), so
    both sides run to epsilon = 1e-8.  At that epsilon the energy the reference REPORTS (stale G, rhf.rs:84-85) is first order in the
    residual - the two reported values agree to a few 1e-8, depending on where each side stops - so the parity statement is the
    variational energy of the two converged densities, which is second order, evaluated by the oracle for both sides."""
    import os
    q, s, o = _sys("benzene", "cc-pVDZ")
    I, _ = o.eri_strided_mt(0, 1, min(16, len(os.sched_getaffinity(0))))
    ref = o.rhf(100, 1e-8, eri=I)
    assert ref["status"] == 0
    st = q.ScfStepper(s)
    e = rms = None
    for k in range(101):
        e, rms = st.iterate()
        if rms < 1e-8:
            break
    assert rms < 1e-8 and abs(k - ref["iterations"]) <= 3
    D = st.density(0)
    H = st.matrix("H")
    st.close()
    evar = lambda P: 0.5 * np.sum(P * (2 * H + o.g_rhf(P, I)))
    assert abs(evar(D) - evar(ref["density"])) < 1e-9
    assert abs(e + s.nuclear_repulsion() - ref["total_energy"]) < 5 * TOL_E          # plausibility bound on the reported values
    out = q.restricted_hartree_fock(s, q.HartreeFockConfig(100, 1e-8))              # the driver returns what the stepper saw
    assert out is not None and out.iterations == k and out.electronic_energy == e


def test_benzene_ccpvdz_reaches_the_noise_floor():
    """BASELINE config 5 at epsilon = 1e-10: the loop of rhf.rs:66-104 - never-reset DIIS over six samples - has a noise floor
    on this molecule; the pass at which rms first dips below 1e-10 is random (24, 30, 87, > 95 in five variants of the product; the oracle
    stalls at 3e-9).  What IS robust, and pinned here: the floor is reached by pass 21 (rms < 1e-9), the walk stays orders of magnitude
    below the convergence region's entry (< 1e-5 through pass 60; excursions depend on the last bits of G - 3e-8 with round 3's work
    lists, 1.5e-6 with round 4's, whose cost-sorted order differs - a bound of 1e-7 is NOT robust), and the energy no longer moves: the
    reported one (stale G: first order in the residual - 1.2e-7 Eh off in the two passes of an excursion) to 1e-6 Eh, the variational one
    of the pass's density, evaluated by a second handle's Fock build, to 1e-10."""
    import qchem_rs_amd as q
    m = load_system("benzene", "cc-pVDZ")
    s, s2 = q.System(m), q.System(m)
    st = q.ScfStepper(s)
    H = None
    tr, evar = [], {}
    for k in range(61):
        e, r = st.iterate()
        tr.append((e, r))
        if k in (21, 30, 40, 50, 60):
            if H is None:
                H = st.matrix("H")
            D = st.density(0)
            evar[k] = 0.5 * float(np.sum(D * (2 * H + s2.fock_rhf(D))))
    st.close(); s.close(); s2.close()
    first = next(k for k, (_, r) in enumerate(tr) if r < 1e-9)
    assert first <= 21, first
    assert max(r for _, r in tr[21:]) < 1e-5
    assert max(abs(e - tr[21][0]) for e, _ in tr[21:]) < 1e-6
    ev = list(evar.values())
    assert max(ev) - min(ev) < 1e-10, evar


@pytest.mark.parametrize("mol,basis", [("water", "cc-pVDZ"), ("ethylene", "6-31G_st_st"), ("oxygen", "cc-pVDZ")])
def test_startup_stages_match_oracle(mol, basis):
    """X = S^-1/2 with the diagonal-of-the-product quirk (rhf.rs:124-131), H = T + V and the Hueckel density with the
    1.75-scaled diagonal (rhf.rs:133-150) - stage by stage against the oracle's orc_core_guess."""
    q, s, o = _sys(mol, basis)
    S_ref, H_ref, X_ref, D_ref = o.core_guess()
    st = q.ScfStepper(s)
    assert np.abs(st.matrix("S") - S_ref).max() < 1e-11
    assert np.abs(st.matrix("H") - H_ref).max() < 1e-10 * max(1.0, np.abs(H_ref).max())
    assert np.abs(st.matrix("X") - X_ref).max() < 1e-9 * max(1.0, np.abs(X_ref).max())
    D0 = st.density(0)
    st.close()
    if mol != "oxygen":          # homonuclear: degenerate Hueckel orbitals on the occupation boundary make D0 eigensolver-dependent
        assert np.abs(D0 - D_ref).max() < 1e-8 * max(1.0, np.abs(D_ref).max())
    assert abs(np.sum(D0 * S_ref) - 2 * (s.n_electrons() // 2)) < 1e-9          # tr(D S) = N


@pytest.mark.parametrize("mol,basis", [("water", "cc-pVDZ"), ("ethylene", "STO-3G"), ("water", "cc-pVTZ"), ("ethylene", "6-31G_st_st")])
def test_rhf_passes_match_oracle_one_by_one(mol, basis):
    """Every pass of the loop body (rhf.rs:67-88) against the oracle's trace: energy and density rms of pass k agree, so guess,
    DIIS window growth (passthrough below 4 samples, extrapolation from the 4th on, diis.rs:28-59), eigensolve and density
    update are each pinned - not only the converged end point.  (water / cc-pVTZ is BASELINE's headline configuration: f shells, the
    one-workgroup Roothaan kernel with its tridiagonal and refinement eigensolves, 8 launches on the dispatch lanes.)"""
    q, s, o = _sys(mol, basis)
    ref = o.rhf(100, 1e-10, trace=True)
    st = q.ScfStepper(s)
    for k in range(len(ref["trace_energy"])):
        e, rms = st.iterate()
        assert abs(e - ref["trace_energy"][k]) < 1e-9 * max(1.0, abs(e)), k
        assert abs(rms - ref["trace_rms"][k]) < 1e-9 + 1e-5 * ref["trace_rms"][k], k
    st.close()


@pytest.mark.parametrize("mol,basis", [("water", "STO-3G"), ("water", "cc-pVTZ"), ("ethylene", "6-31G_st_st")])
def test_stored_tensor_mode_rhf(mol, basis):
    """The reference's own conventional algorithm on the GPU (tensor + electron_terms resident in HBM, GEMV per pass)."""
    q, s, o = _sys(mol, basis)
    s.set_fock_mode("stored")
    out = q.restricted_hartree_fock(s, q.HartreeFockConfig(100, 1e-10))
    ref = o.rhf(100, 1e-10)
    assert out is not None and abs(out.total_energy() - ref["total_energy"]) < TOL_E
    assert out.iterations == ref["iterations"]
    s.set_fock_mode("direct")
    out2 = q.restricted_hartree_fock(s, q.HartreeFockConfig(100, 1e-10))
    assert abs(out2.total_energy() - out.total_energy()) < 1e-9


def test_stored_tensor_mode_uhf_triplet():
    q, s, o = _sys("oxygen", "cc-pVDZ")
    s.set_fock_mode("stored")
    st = q.ScfStepper(s, uhf=True, n_alpha=9, n_beta=7)
    s.set_fock_mode("direct")
    st2 = q.ScfStepper(s, uhf=True, n_alpha=9, n_beta=7)
    for _ in range(6):                       # pass-by-pass agreement of the two Fock modes (open shell: Da != Db)
        e1, r1 = st.iterate(); e2, r2 = st2.iterate()
        assert abs(e1 - e2) < 1e-9 * max(1.0, abs(e2)) and abs(r1 - r2) < 1e-9 + 1e-6 * r2
    st.close(); st2.close()


@pytest.mark.parametrize("mol,basis,uhf", [("water", "cc-pVTZ", False), ("ethylene", "cc-pVDZ", False), ("water", "6-31G_st_st", True),
                                           ("hydrogen", "STO-3G", False), ("oxygen", "cc-pVDZ", True)])
def test_fused_small_roothaan_step_equals_the_generic_launch_sequence(mol, basis, uhf, monkeypatch):
    """qc_scf_small.hip (n <= 64: the whole Roothaan step of rhf.rs:70-88 in one workgroup, matrices in LDS) against the generic
    sequence of launches it replaces (QC_NO_SMALL_FUSED=1): same passes, same energies, both against the oracle.  Covers the
    one-tile-per-wave form (n <= 32), the 2 x 2 form (n = 48, 58), the DIIS windows of RHF (4, 6) and UHF (2, 8), and the cold
    (tridiagonal / Jacobi start) and warm (refinement) eigensolves."""
    q, s, o = _sys(mol, basis)
    run = q.unrestricted_hartree_fock if uhf else q.restricted_hartree_fock
    cfg = q.HartreeFockConfig(100, 1e-10)
    fused = run(s, cfg)
    monkeypatch.setenv("QC_NO_SMALL_FUSED", "1")
    generic = run(s, cfg)
    monkeypatch.delenv("QC_NO_SMALL_FUSED")
    ref = (o.uhf if uhf else o.rhf)(100, 1e-10)
    assert fused is not None and generic is not None and ref["status"] == 0
    assert abs(fused.total_energy() - generic.total_energy()) < 1e-10
    assert abs(fused.total_energy() - ref["total_energy"]) < TOL_E
    assert abs(fused.iterations - generic.iterations) <= 1
    wa = fused.orbital_energies_alpha if uhf else fused.orbital_energies
    wb = generic.orbital_energies_alpha if uhf else generic.orbital_energies
    assert np.abs(np.array(wa) - np.array(wb)).max() < 1e-8
    # the fused path is deterministic: a second run repeats the first bit for bit
    again = run(s, cfg)
    assert again.electronic_energy == fused.electronic_energy and again.iterations == fused.iterations


def test_not_converged_returns_none():
    q, s, o = _sys("water", "STO-3G")
    assert q.restricted_hartree_fock(s, q.HartreeFockConfig(max_iterations=1, epsilon=1e-14)) is None


def test_cli_rhf_and_uhf_end_to_end(capsys):
    """`qchem-hip`: the reference's command line through the loaders, the C ABI and the kernels; the printed
    three-decimal values are the oracle's, the opt-in extension (charge / multiplicity) reports <S^2> of triplet O2."""
    import os
    import qchem_rs_amd  # noqa: F401
    from qchem_rs_amd import cli
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    b = lambda n: os.path.join(root, "data", "basis", n + ".json")
    m = lambda n: os.path.join(root, "data", "mol", n + ".json")
    q, s, o = _sys("water", "STO-3G")
    ref = o.rhf(100, 1e-6)
    s.close()
    assert cli.main(["rhf", "-b", b("STO-3G"), "-m", m("water")]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith("hartree fock converged after %d iterations and " % ref["iterations"])
    assert lines[3] == "hartree fock energy: %.3f" % ref["total_energy"]
    assert lines[4] == "orbital energies: [" + ", ".join("%.3f" % w for w in ref["orbital_energies"]) + "]"
    assert cli.main(["uhf", "-b", b("cc-pVDZ"), "-m", m("oxygen"), "-s", "3", "--json"]) == 0
    lines = capsys.readouterr().out.splitlines()
    import json
    doc = json.loads(lines[-1])
    assert (doc["n_alpha"], doc["n_beta"]) == (9, 7) and 2.0 < doc["spin_square"] < 2.1
    q, s, o = _sys("oxygen", "cc-pVDZ")
    ref = o.uhf(100, 1e-6, n_alpha=9, n_beta=7)
    s.close()
    # (the triplet crawls on a saddle of the UHF functional and amplifies rounding differences about tenfold per pass - see
    # test_uhf_triplet_oxygen_extension; at the CLI's default epsilon = 1e-6 the stopping pass and the sixth decimal of the
    # reported energy therefore depend on the eigensolver's last bits.  What the command line prints - three decimals - does not.)
    assert lines[-2].startswith("<S^2>: 2.0") and abs(doc["total_energy"] - ref["total_energy"]) < 1e-4
    assert abs(doc["iterations"] - ref["iterations"]) <= 3
    assert cli.main(["rhf", "-b", b("STO-3G"), "-m", m("water"), "--max-iterations", "1", "--epsilon", "1e-14"]) == 101


def test_fock_cartesian_f_shells_wide_ket_blocks():
    """Every shell of water/cc-pVTZ taken as Cartesian (n = 65): f.f pairs have 100 function pairs - more than the 64 lanes of a
    group, so the matrix-core classes run their second column pass and the 64-lane digestion its wide-block branches - and d.d
    pairs 36.  G (RHF and UHF) against the dense contraction of the oracle's tensor for the same shells."""
    import qchem_rs_amd as q
    from oracle.oracle import Oracle
    m = load_system("water", "cc-pVTZ")
    m.shell_pure[:] = 0
    s, o = q.System(m), Oracle(m)
    assert s.n == 65
    I = o.eri()
    D = _rand_sym(s.n, 5)
    G_ref = o.g_rhf(D, I)
    scale = max(1.0, np.abs(G_ref).max())
    assert np.abs(s.fock_rhf(D) - G_ref).max() < TOL_INT * scale
    Da, Db = _rand_sym(s.n, 6), _rand_sym(s.n, 7)
    Ga, Gb = s.fock_uhf(Da, Db)
    assert np.abs(Ga - o.g_uhf(Da, Db, I)).max() < TOL_INT * scale
    assert np.abs(Gb - o.g_uhf(Db, Da, I)).max() < TOL_INT * scale
    assert np.abs(s.eri() - I).max() < TOL_INT
    s.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# Shapes above n = 64: Fock builds against the oracle's contraction of the complete quartet list, the rotation eigensolvers at every
# size regime, open-shell SCF on the generic launch sequence.

def _jk_refs(o, Da, Db):
    """RHF G(Da), UHF G_alpha and G_beta of every unique shell quartet, from the oracle's J and K (orc_jk_quartets): J is linear in
    the density, so two contractions serve all three - G = J(Da) - K(Da)/2, G_a = J(Da + Db) - K(Da), G_b = J(Da + Db) - K(Db)."""
    Ja, Ka = o.jk_all_quartets(Da, Da)
    Jb, Kb = o.jk_all_quartets(Db, Db)
    return Ja - 0.5 * Ka, Ja + Jb - Ka, Ja + Jb - Kb


def _column_classes(s, n):
    """{class id: quartets} of one instrumented build (qc_fock_profile; id = (BM << 12) | (LAB << 8) | (LCD << 4) | LGC).  The device
    buffers come from the HIP runtime the library is bound to: the system's, or - if torch was loaded first - the copy torch bundles
    (a second runtime in the process may not find the device once the first has opened it)."""
    import ctypes as C
    import sys
    import qchem_rs_amd as q
    q.hf.lib()
    other = os.path.dirname(sys.modules["torch"].__file__) if "torch" in sys.modules else None
    with open("/proc/self/maps") as f:
        paths = sorted({l.split()[-1] for l in f if "libamdhip64.so" in l})
    hip = C.CDLL(([p for p in paths if not (other and p.startswith(other))] or paths)[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    D = np.ascontiguousarray(_rand_sym(n, 0))
    dD, dG = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dD), D.nbytes) == 0 and hip.hipMalloc(C.byref(dG), D.nbytes) == 0
    try:
        assert hip.hipMemcpy(dD, D.ctypes.data_as(C.c_void_p), D.nbytes, 1) == 0          # hipMemcpyHostToDevice
        assert hip.hipMemset(dG, 0, D.nbytes) == 0
        pr = s.fock_profile(dD.value, dG.value, 1)
    finally:
        hip.hipFree(dD); hip.hipFree(dG)
    return {int(c): int(k) for c, k in zip(pr["class_id"], pr["quartets"])}


def _valu_fket_quartets(classes):
    """Quartets of the d.d / f.p-ket column classes (LCD = 4) with a d.p ... f.f bra (LAB >= 3) in their 32-lane VALU form (LGC = 5) -
    the lists longer than QC_MFMA4_MAX (qc_plan.cpp); shorter ones run as matrix-core tiles in the 64-lane instance (LGC = 6)."""
    return [k for c, k in classes.items() if not c >> 12 and (c >> 8) & 15 >= 3 and (c >> 4) & 15 == 4 and c & 15 == 5]


@pytest.mark.parametrize("mol,basis", [("benzene", "6-311++G_st_st"), ("ethylene", "cc-pVTZ"), ("benzene", "cc-pVDZ")])
def test_fock_above_n64_matches_the_oracle_quartet_contraction(mol, basis):
    """RHF G and UHF G_alpha, G_beta (Da != Db) at n = 174 (benzene/6-311++G**: diffuse sp shells, 8.4 M quartets, beyond every in-LDS
    eigensolver), 116 (ethylene/cc-pVTZ: f functions in a build above the bra-major merge limit, d.p / f.s and d.d / f.p bras whose
    d.d / f.p-ket lists are too long for the matrix-core form) and 114 (benzene/cc-pVDZ: UHF with the bra-major workgroups' LDS rows
    sized for two spins) against the oracle's J and K of the complete unique quartet list - built on the oracle side, not from the
    product's plan - and bitwise repeatable on the same handle."""
    q, s, o = _sys(mol, basis)
    assert s.n > 64
    if basis == "cc-pVTZ":
        assert max(_valu_fket_quartets(_column_classes(s, s.n)), default=0) > 1024, "the VALU route of the f-basis build is gone"
    Da, Db = _rand_sym(s.n, 71), _rand_sym(s.n, 72)
    G = s.fock_rhf(Da)
    Ga, Gb = s.fock_uhf(Da, Db)
    G_ref, Ga_ref, Gb_ref = _jk_refs(o, Da, Db)
    for X, R in ((G, G_ref), (Ga, Ga_ref), (Gb, Gb_ref)):
        assert np.abs(X - R).max() < TOL_INT * max(1.0, np.abs(R).max())
    assert np.array_equal(s.fock_rhf(Da), G)
    Ga2, Gb2 = s.fock_uhf(Da, Db)
    assert np.array_equal(Ga2, Ga) and np.array_equal(Gb2, Gb)
    s.close()


@pytest.mark.parametrize("which", ["water", "oxygen-cartesian"])
def test_fock_f_basis_valu_route_on_small_systems(which, monkeypatch, tmp_path):
    """QC_MFMA4_MAX = 0 (read per system): every d.d / f.p-ket list of a d.p ... f.f bra takes the 32-lane VALU form inside the
    f-capable wide-ket kernels - the route of long lists (ethylene/cc-pVTZ and larger) - on water/cc-pVTZ and on O2/cc-pVTZ with
    Cartesian d and f shells, where the dense tensor is cheap.  RHF and UHF against the dense contraction, bitwise repeatable."""
    import json
    import qchem_rs_amd as q
    from oracle.oracle import Oracle
    from conftest import data
    if which == "water":
        m = load_system("water", "cc-pVTZ")
    else:
        b = json.load(open(data("basis", "cc-pVTZ.json")))
        for el in b["elements"].values():
            for sh in el["electron_shells"]:
                if sh["angular_momentum"][0] >= 2:
                    sh["function_type"] = "gto_cartesian"
        f = tmp_path / "cc-pVTZ-cart.json"
        f.write_text(json.dumps(b))
        m = q.MolecularSystem.load(data("mol", "oxygen.json"), q.BasisSet.load(str(f)))
    o = Oracle(m)
    s_def = q.System(m)
    nq_def = sum(_valu_fket_quartets(_column_classes(s_def, s_def.n)))
    s_def.close()
    monkeypatch.setenv("QC_MFMA4_MAX", "0")
    s = q.System(m)
    monkeypatch.delenv("QC_MFMA4_MAX")
    nq = sum(_valu_fket_quartets(_column_classes(s, s.n)))
    assert nq > nq_def, (nq, nq_def)
    I = o.eri()
    D, Da, Db = _rand_sym(s.n, 81), _rand_sym(s.n, 82), _rand_sym(s.n, 83)
    G_ref = o.g_rhf(D, I)
    G = s.fock_rhf(D)
    assert np.abs(G - G_ref).max() < TOL_INT * max(1.0, np.abs(G_ref).max())
    Ga, Gb = s.fock_uhf(Da, Db)
    Ga_ref, Gb_ref = o.g_uhf(Da, Db, I), o.g_uhf(Db, Da, I)
    assert np.abs(Ga - Ga_ref).max() < TOL_INT * max(1.0, np.abs(Ga_ref).max())
    assert np.abs(Gb - Gb_ref).max() < TOL_INT * max(1.0, np.abs(Gb_ref).max())
    assert np.array_equal(s.fock_rhf(D), G)
    Ga2, Gb2 = s.fock_uhf(Da, Db)
    assert np.array_equal(Ga2, Ga) and np.array_equal(Gb2, Gb)
    s.close()


@pytest.mark.parametrize("n", [24, 64, 100, 101, 114, 128, 129, 174, 230])
def test_rotation_eigensolvers_at_every_size_regime(n):
    """The single-workgroup Jacobi kernels of qc_eig_device - two-sided with A and V in LDS up to n = 100 (qc_jacobi_kernel<true>),
    one-sided in LDS for 101..128 (qc_jacobi1_kernel), one-sided in global memory above (qc_jacobi1g_kernel) - every eigensolve of
    open-shell UHF and the fallback of the tridiagonal path.  Reached through sym_eig_warm(A, I): the refinement finds a dense A far
    from diagonal (emax > 0.1), falls back to rotations on X^T A X = A exactly, and V = I Q is exact.  Dense random spectra and
    Q diag(w) Q^T with exactly repeated eigenvalues and 1e-9 clusters, with the bars of test_sym_eig; at n = 114 and 174 also the
    near-eigenvector start of an open-shell pass (perturbation 0.3), with the bars of test_sym_eig_warm_start_regimes."""
    import qchem_rs_amd as q
    s = q.System(load_system("hydrogen", "STO-3G"))
    rng = np.random.default_rng(500 + n)
    d = np.sort(rng.uniform(-10, 10, n))
    for k in range(0, n - 7, 12):
        d[k + 1] = d[k]                                        # exactly repeated
        d[k + 5] = d[k + 4] + 1e-9; d[k + 6] = d[k + 4] + 2e-9     # a 1e-9 cluster
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A2 = (Q * d) @ Q.T; A2 = 0.5 * (A2 + A2.T)
    for A in (_rand_sym(n, 900 + n), A2):
        V, w = s.sym_eig_warm(A, np.eye(n))
        w_ref = np.linalg.eigvalsh(A)
        assert np.all(np.diff(w) >= 0)
        assert np.abs(w - w_ref).max() < 1e-12 * max(1.0, np.abs(w_ref).max())
        assert np.abs(V.T @ V - np.eye(n)).max() < 1e-12
        assert np.abs(A @ V - V * w).max() < 1e-11 * max(1.0, np.abs(w_ref).max())
    if n in (114, 174):
        _, V0 = np.linalg.eigh(A2)
        P = rng.standard_normal((n, n)); B = A2 + 0.3 * (P + P.T)
        V, w = s.sym_eig_warm(B, V0)
        assert np.all(np.diff(w) >= 0)
        assert np.abs(w - np.linalg.eigvalsh(B)).max() < 1e-11
        assert np.abs(V.T @ V - np.eye(n)).max() < 1e-12
        assert np.abs(B @ V - V * w).max() < 1e-10
    s.close()


@pytest.mark.parametrize("basis", ["6-311++G_st_st", "cc-pVTZ"])
def test_open_shell_passes_above_n64_match_oracle(basis):
    """Triplet ethylene (n_alpha = 9, n_beta = 7) at n = 72 (6-311++G**: the generic launch sequence - GEMMs, device DIIS - with the
    two-sided rotation kernel) and n = 116 (cc-pVTZ: f functions, the one-sided LDS rotation kernel) pass by pass against the oracle's
    trace.  The oracle does not converge either case in 200 passes (never-reset DIIS, as for O2), so the first 12 passes are compared,
    with the open-shell bars of test_uhf_passes_match_oracle_one_by_one; pass 0 to 1e-9.  Then <S^2> against numpy on the densities,
    and a second run repeats the first bit for bit."""
    q, s, o = _sys("ethylene", basis)
    assert s.n > 64
    I, _ = o.eri_strided_mt(0, 1, min(16, len(os.sched_getaffinity(0))))
    ref = o.uhf(12, 1e-30, n_alpha=9, n_beta=7, eri=I, trace=True)
    del I
    assert len(ref["trace_energy"]) >= 12

    def run():
        st = q.ScfStepper(s, uhf=True, n_alpha=9, n_beta=7)
        tr = [st.iterate() for _ in range(12)]
        out = tr, st.density(0), st.density(1), st.spin_square()
        st.close()
        return out

    tr, Da, Db, s2 = run()
    for k, (e, rms) in enumerate(tr):
        tol = 1e-9 if k == 0 else 1e-7
        assert abs(e - ref["trace_energy"][k]) < tol * max(1.0, abs(e)), k
        if k == 0:
            assert abs(rms - ref["trace_rms"][0]) < 1e-9 * max(1.0, ref["trace_rms"][0])
        else:
            assert abs(rms - ref["trace_rms"][k]) < tol + 1e-4 * ref["trace_rms"][k], k
    S = o.overlap()
    assert abs(s2 - (1.0 * 2.0 + 7 - np.trace(Da @ S @ Db @ S))) < 1e-10
    tr2, Da2, Db2, s2b = run()
    assert tr2 == tr and np.array_equal(Da2, Da) and np.array_equal(Db2, Db) and s2b == s2
    s.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# The materialised tensor above n = 64 (qc_eri_full: the tensor behind MP2 and the stored Fock mode) and the stored-tensor SCF in every
# launch form of qc_tensor_gemv, against the oracle.

def _oracle_tensor(o):
    I, _ = o.eri_strided_mt(0, 1, min(16, len(os.sched_getaffinity(0))))
    return I


def _pp_bm_unit(q):
    names = [u for u in range(q.hf.PROFILE_UNITS) if q.hf.unit_name(u) == "qc_fock_bm_kernel<2, 0>"]
    assert len(names) == 1
    return names[0]


@pytest.mark.parametrize("mol,basis,n", [("chloroform", "6-31G_st_st", 77), ("benzene", "cc-pVDZ", 114), ("ethylene", "cc-pVTZ", 116)])
def test_eri_tensor_above_n64_matches_oracle(mol, basis, n):
    """qc_eri_full element by element against the oracle's tensor at n = 77 (chloroform/6-31G**: Cl, odd n), 114 (benzene/cc-pVDZ: its
    p.p-ket bra-major class, which tensor mode hands to the column kernels) and 116 (ethylene/cc-pVTZ: f functions, d.d / f.p-ket lists
    in their 32-lane VALU form, LGC = 5) - compared one slab of the first index at a time.  The 8 symmetry images agree to rounding, and
    a second call on the same handle repeats the first bit for bit (MP2's reproducibility rests on it)."""
    q, s, o = _sys(mol, basis)
    assert s.n == n
    if basis == "cc-pVTZ":
        assert max(_valu_fket_quartets(_column_classes(s, s.n)), default=0) > 1024, "the VALU route of the f-basis tensor is gone"
    if mol == "benzene":
        s.fock_rhf(_rand_sym(n, 0))
        assert s.unit_quartets()[_pp_bm_unit(q)] > 0, "benzene/cc-pVDZ has no p.p-ket bra-major class any more"
    I = s.eri()
    R = _oracle_tensor(o)
    for a in range(n):
        assert np.abs(I[a] - R[a]).max() < TOL_INT, a
    del R
    scale = np.abs(I).max()
    for a in range(n):
        X = I[a]                                                       # X[j, k, l] = (aj|kl)
        assert np.abs(X - I[:, a]).max() <= 1e-14 * scale, a          # (ja|kl)
        assert np.abs(X - X.transpose(0, 2, 1)).max() <= 1e-14 * scale, a        # (aj|lk)
        assert np.abs(X - I[:, :, a, :].transpose(2, 0, 1)).max() <= 1e-14 * scale, a     # (kl|aj)
    assert np.array_equal(s.eri(), I)
    s.close()


@pytest.mark.parametrize("route", ["valu-fket", "pp-bm-to-column"])
def test_eri_tensor_routes_on_small_systems(route, monkeypatch):
    """The tensor-mode stores of two routes the default plans of small systems never take, against the dense oracle tensor:
    QC_MFMA4_MAX = 0 on water/cc-pVTZ (every d.d / f.p-ket list of a d.p ... f.f bra in the 32-lane VALU form, LGC = 5) and
    QC_BM_PP_MIN = 1 on water/cc-pVDZ (p.p-ket bra-major classes, which qc_launch_eri_full runs in the column kernels)."""
    import qchem_rs_amd as q
    from oracle.oracle import Oracle
    mol, basis, var = ("water", "cc-pVTZ", "QC_MFMA4_MAX") if route == "valu-fket" else ("water", "cc-pVDZ", "QC_BM_PP_MIN")
    m = load_system(mol, basis)
    o = Oracle(m)
    monkeypatch.setenv(var, "0" if route == "valu-fket" else "1")
    s = q.System(m)
    monkeypatch.delenv(var)
    if route == "valu-fket":
        assert sum(_valu_fket_quartets(_column_classes(s, s.n))) > 0
    else:
        s.fock_rhf(_rand_sym(s.n, 0))
        assert s.unit_quartets()[_pp_bm_unit(q)] > 0
    I = s.eri()
    assert np.abs(I - o.eri()).max() < TOL_INT
    assert np.array_equal(s.eri(), I)
    s.close()


def _gemv_form(n, nspin):
    """Launch form of qc_tensor_gemv for n and 1 (RHF) or 2 (UHF) tensors: D in LDS within 48 KB, in LDS above 48 KB, or through L2."""
    lds = nspin * (n * n + 1) * 8
    return "lds" if lds <= 48 * 1024 else ("lds-raised" if lds <= 150 * 1024 else "l2")


@pytest.mark.parametrize("mol,basis,n,form", [("benzene", "cc-pVDZ", 114, "lds-raised"), ("benzene", "6-311++G_st_st", 174, "l2")])
def test_stored_tensor_rhf_passes_above_n64(mol, basis, n, form):
    """Stored-tensor RHF (qc_tensor_gemv on T = I - I^x / 2) pass by pass in the GEMV forms with D in LDS above 48 KB (n = 114) and with
    D read through L2 (n = 174), against the direct build on the same handle - which
    test_fock_above_n64_matches_the_oracle_quartet_contraction pins to the oracle at these sizes - and at n = 114 also against the
    oracle's trace on its own tensor (no 7.3 GB oracle SCF at n = 174): energy to 1e-9 relative, rms to 2e-8 + 1e-5 relative - both
    modes are 6.5e-9 from the oracle's rms at pass 11 (measured; benzene's near-degenerate orbitals, see
    test_benzene_ccpvdz_energy_matches_oracle), and 6e-11 from each other.

    benzene/6-311++G**: the Hueckel start in a basis with diffuse shells is poorly conditioned (density rms 1.6e6 after pass 0), so the
    last digits of G - each mode agrees with the oracle to 1e-10 of the largest element - reach the energies of the first passes at up
    to 8e-9 relative and the rms at up to 1e-2 (measured); by pass 8 DIIS has damped them to 1e-10 in the energy and 3e-4 in the rms.
    Bars there: energy 2e-8 relative through pass 7, 1e-9 from pass 8 on; rms 1e-3 relative from pass 8 on."""
    q, s, o = _sys(mol, basis)
    assert s.n == n and _gemv_form(n, 1) == form
    ref = None
    if n <= 128:
        I = _oracle_tensor(o)
        ref = o.rhf(12, 1e-30, eri=I, trace=True)
        del I
        assert len(ref["trace_energy"]) >= 12
    s.set_fock_mode("stored")
    st = q.ScfStepper(s)
    s.set_fock_mode("direct")
    st2 = q.ScfStepper(s)
    for k in range(12):
        e1, r1 = st.iterate(); e2, r2 = st2.iterate()
        if ref is not None:
            assert abs(e1 - ref["trace_energy"][k]) < 1e-9 * max(1.0, abs(e1)), k
            assert abs(r1 - ref["trace_rms"][k]) < 2e-8 + 1e-5 * ref["trace_rms"][k], k
            assert abs(e1 - e2) < 1e-9 * max(1.0, abs(e2)), k
            assert abs(r1 - r2) < 1e-9 + 1e-6 * r2, k
        elif k < 8:
            assert abs(e1 - e2) < 2e-8 * abs(e2), k
        else:
            assert abs(e1 - e2) < 1e-9 * abs(e2), k
            assert abs(r1 - r2) < 1e-3 * r2, k
    st.close(); st2.close(); s.close()


@pytest.mark.parametrize("mol,basis,n,na,nb,form", [("chloroform", "6-31G_st_st", 77, 30, 28, "lds-raised"),
                                                    ("ethylene", "cc-pVTZ", 116, 9, 7, "l2")])
def test_stored_tensor_uhf_passes_match_oracle_above_n64(mol, basis, n, na, nb, form):
    """Stored-tensor UHF (two tensors, I and its exchange permutation, Da != Db) pass by pass against the oracle's trace on its own tensor:
    triplet chloroform at n = 77 (D in LDS above 48 KB, odd n: the n^2 tail of the GEMV) and triplet ethylene at n = 116 (D through L2).
    The first 12 passes, with the bars of test_open_shell_passes_above_n64_match_oracle."""
    q, s, o = _sys(mol, basis)
    assert s.n == n and _gemv_form(n, 2) == form
    I = _oracle_tensor(o)
    ref = o.uhf(12, 1e-30, n_alpha=na, n_beta=nb, eri=I, trace=True)
    del I
    assert len(ref["trace_energy"]) >= 12
    s.set_fock_mode("stored")
    st = q.ScfStepper(s, uhf=True, n_alpha=na, n_beta=nb)
    for k in range(12):
        e, rms = st.iterate()
        tol = 1e-9 if k == 0 else 1e-7
        assert abs(e - ref["trace_energy"][k]) < tol * max(1.0, abs(e)), k
        if k == 0:
            assert abs(rms - ref["trace_rms"][0]) < 1e-9 * max(1.0, ref["trace_rms"][0])
        else:
            assert abs(rms - ref["trace_rms"][k]) < tol + 1e-4 * ref["trace_rms"][k], k
    st.close(); s.close()
