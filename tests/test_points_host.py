"""Host tests of the values on points: the new entry points are declared, listed, exported and bound in the Rust source; the two host-only
ones (qc_basis_on_points, qc_potential_matrix) against the references of tests/points_reference.py; the self-checks of those references;
the argument checks that run before any device is touched; the CLI's --cube parsing and file format.

Systems: the four of test_dipole_host.SYSTEMS (n = 64, 80, 18, 58; every s..f pair class, pure and Cartesian, 169 primitive pairs in one
shell pair).  Bounds: phi <= 1e-13 max(1, max|phi|) (unit-norm functions; the sums have at most 13 primitives and 10 monomials);
A <= 1e-12 max(1, max|A|), the margin of the existing host-vs-oracle nuclear-attraction test.

Measured on the CPU (40 points per system for A):
  system          n   max|phi_host - phi_numpy|  max|phi|  max|A_host - A_oracle|  max|A|
  tetra-pure-2    64  3.3e-16                    1.45      1.1e-15                 2.48
  tetra-cart-1    80  3.3e-16                    0.90      8.9e-16                 1.78
  deep            18  7.1e-15                    51.6      5.3e-15                 14.4
  water/cc-pVTZ   58  1.8e-15                    11.9      7.8e-16                 7.64
Reference self-checks: sum_A Z_A [-tr(D A(R_A))] vs tr(D qc_nuclear) on water/cc-pVTZ: relative 2.3e-14 (bound 1e-11); the H2/STO-3G
oracle RHF density on the cube grid (spacing 0.2, margin 4.0) integrates to 1.99924 (bound: 2 +- 2e-3)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, data, load_system
import points_reference as PR
import synthetic_systems as Y
from test_dipole_host import SYSTEMS

NEW = ("qc_basis_on_points", "qc_potential_matrix", "qc_esp_records", "qc_density_on_points", "qc_esp_on_points", "qc_orbitals_on_points",
       "qc_scf_density_on_points", "qc_scf_esp_on_points", "qc_scf_orbitals_on_points", "qc_points_timings")
NREF = 40            # points per system with an oracle potential matrix


def test_point_entry_points_are_declared_listed_exported_and_bound():
    import qchem_rs_amd as q
    header = open(os.path.join(ROOT, "include", "qchem_hip.h")).read()
    declared = set(re.findall(r"\b(qc_[a-z0-9_]+)\s*\(", header))
    ffi = open(os.path.join(ROOT, "bindings", "rust", "qchem-hip", "src", "ffi.rs")).read()
    L = q.lib()
    for name in NEW:
        assert name in declared, name
        assert name in q.hf.EXPORTS, name
        assert hasattr(L, name), name
        assert "pub fn %s(" % name in ffi, name
    for cls, names in ((q.System, ("basis_on_points", "potential_matrix", "density_on_points", "esp_on_points", "orbitals_on_points")),
                       (q.ScfStepper, ("density_on_points", "esp_on_points", "orbitals_on_points"))):
        for name in names:
            assert callable(getattr(cls, name)), name


@pytest.fixture(scope="module")
def computed():
    """per system: the sample points, phi from numpy and from the host entry, A from the oracle and from the host entry on NREF points"""
    import qchem_rs_amd as q
    out = {}
    for k, (name, make) in enumerate(SYSTEMS.items()):
        m = make()
        P = PR.sample_points(m, 100 + k)
        s = q.System(m)
        out[name] = dict(m=m, P=P, phi_ref=PR.phi(m, P), phi=s.basis_on_points(P),
                         A_ref=np.array([PR.potential_matrix_oracle(m, r) for r in P[:NREF]]), A=np.array([s.potential_matrix(r) for r in P[:NREF]]))
        s.close()
    return out


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_host_basis_values_match_numpy(computed, name):
    c = computed[name]
    err, scale = float(np.abs(c["phi"] - c["phi_ref"]).max()), float(np.abs(c["phi_ref"]).max())
    print(name, "max|phi_host - phi_numpy|", err, "max|phi|", scale)
    assert c["phi"].shape == (PR.NPOINTS, c["m"].n_basis())
    assert err <= 1e-13 * max(1.0, scale)


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_host_potential_matrix_matches_the_oracle_and_is_exactly_symmetric(computed, name):
    c = computed[name]
    err, scale = float(np.abs(c["A"] - c["A_ref"]).max()), float(np.abs(c["A_ref"]).max())
    print(name, "max|A_host - A_oracle|", err, "max|A|", scale)
    assert err <= 1e-12 * max(1.0, scale)
    assert np.array_equal(c["A"], c["A"].transpose(0, 2, 1)) and np.array_equal(c["A_ref"], c["A_ref"].transpose(0, 2, 1))
    assert np.all(np.einsum("kaa->ka", c["A"]) > 0)                     # (a| 1/r |a) of a real function is positive


def test_reference_potential_reproduces_the_nuclear_attraction_trace():
    """sum_A Z_A [-tr(D A(R_A))] = tr(D V): the oracle route's sign and its unit charge, against the library's host V"""
    import qchem_rs_amd as q
    m = load_system("water", "cc-pVTZ")
    s = q.System(m)
    D = Y.rand_sym(s.n, 5)
    want = float(np.sum(D * s.nuclear()))
    got = sum(-float(a.ordinal) * float(np.sum(D * PR.potential_matrix_oracle(m, a.position))) for a in m.atoms)
    print("tr(D V)", want, "from the oracle's point potentials", got, "relative", abs(got - want) / abs(want))
    s.close()
    assert abs(got - want) <= 1e-11 * abs(want)


def _h2_sto3g():
    import qchem_rs_amd as q
    b = q.BasisSet.load(data("basis", "STO-3G.json"))
    return q.MolecularSystem.load(data("mol", "hydrogen.json"), b)


def test_reference_density_of_h2_integrates_to_two_electrons_on_the_cube_grid():
    from oracle.oracle import Oracle
    from qchem_rs_amd import cli
    m = _h2_sto3g()
    o = Oracle(m)
    S, H, I = o.overlap(), o.kinetic() + o.nuclear(), o.eri()
    # two functions, one occupied orbital fixed by symmetry: the bonding combination, normalised
    c = np.ones(2) / np.sqrt(2.0 + 2.0 * S[0, 1])
    Dm = 2.0 * np.outer(c, c)
    F = H + np.einsum("abcd,cd->ab", I, Dm) - 0.5 * np.einsum("acbd,cd->ab", I, Dm)
    assert abs((F @ c - (c @ F @ c) * (S @ c))).max() < 1e-12              # it IS the RHF orbital
    origin, shape, pts = cli.cube_grid(m, 0.2, 4.0)
    phi = PR.phi(m, pts)
    total = float(np.einsum("ka,ab,kb->", phi, Dm, phi) * 0.2 ** 3)
    print("grid", shape, "origin", origin, "integral", total)
    assert shape == [41, 41, 48] and np.allclose(origin, [-4.0, -4.0, -4.0])
    assert abs(total - 2.0) <= 2e-3


def _f(name, *argtypes):
    import qchem_rs_amd as q
    return ctypes.CFUNCTYPE(ctypes.c_int, *argtypes)((name, q.lib()))


vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


def test_argument_errors_are_reported_before_the_device():
    import qchem_rs_amd as q
    INV, OK = q.hf.QC_ERR_INVALID, q.hf.QC_OK
    s = q.System(load_system("water", "STO-3G"))
    n, h = s.n, s.handle
    D, P, out = np.zeros((n, n)), np.zeros((4, 3)), np.zeros(4 * n * n)
    d, p, o = D.ctypes.data, P.ctypes.data, out.ctypes.data
    basis = _f("qc_basis_on_points", vp, i64, vp, vp)
    assert basis(None, 4, p, o) == INV and basis(h, 4, None, o) == INV and basis(h, 4, p, None) == INV and basis(h, -1, p, o) == INV
    assert basis(h, 0, p, o) == OK
    pot = _f("qc_potential_matrix", vp, vp, vp)
    assert pot(None, p, o) == INV and pot(h, None, o) == INV and pot(h, p, None) == INV
    recs = _f("qc_esp_records", vp, vp)
    assert recs(None, o) == INV and recs(h, None) == INV
    dens = _f("qc_density_on_points", vp, vp, i64, vp, vp)
    assert dens(None, d, 4, p, o) == INV and dens(h, None, 4, p, o) == INV and dens(h, d, 4, None, o) == INV and dens(h, d, 4, p, None) == INV
    assert dens(h, d, -1, p, o) == INV
    esp = _f("qc_esp_on_points", vp, vp, i64, vp, vp, vp)
    assert esp(None, d, 4, p, o, None) == INV and esp(h, None, 4, p, o, None) == INV and esp(h, d, 4, None, o, None) == INV
    assert esp(h, d, 4, p, None, None) == INV and esp(h, d, -1, p, o, None) == INV
    orb = _f("qc_orbitals_on_points", vp, ci, vp, i64, vp, vp)
    assert orb(None, 1, d, 4, p, o) == INV and orb(h, 1, None, 4, p, o) == INV and orb(h, 1, d, 4, None, o) == INV and orb(h, 1, d, 4, p, None) == INV
    assert orb(h, 0, d, 4, p, o) == INV and orb(h, -2, d, 4, p, o) == INV and orb(h, 1, d, -1, p, o) == INV
    assert _f("qc_scf_density_on_points", vp, ci, i64, vp, vp)(None, 0, 4, p, o) == INV
    assert _f("qc_scf_esp_on_points", vp, i64, vp, vp, vp)(None, 4, p, o, None) == INV
    assert _f("qc_scf_orbitals_on_points", vp, ci, ci, ci, i64, vp, vp)(None, 0, 0, 1, 4, p, o) == INV
    tim = _f("qc_points_timings", vp, vp)
    assert tim(None, o) == INV and tim(h, None) == INV and tim(h, o) == OK
    # an empty call is fine with or without a device, and writes nothing
    out[:] = 7.0
    assert dens(h, d, 0, p, o) == OK and esp(h, d, 0, p, o, o) == OK and orb(h, 1, d, 0, p, o) == OK
    assert np.all(out == 7.0)
    with pytest.raises(q.QcError, match="reshape"):
        s.basis_on_points(np.zeros(4))
    assert s.basis_on_points(np.zeros((0, 3))).shape == (0, n)
    rec = s.esp_records()                                                   # s and p shells only: pair orders 0..2
    assert rec.shape == (7,) and np.all(rec[:3] > 0) and np.all(rec[3:] == 0)
    s.close()


def test_point_calls_without_a_device_return_no_device_and_invalid_arguments_win():
    import qchem_rs_amd as q
    if q.device_ready():
        pytest.skip("GPU present")
    NODEV, INV = q.hf.QC_ERR_NO_DEVICE, q.hf.QC_ERR_INVALID
    s = q.System(load_system("water", "STO-3G"))
    n, h = s.n, s.handle
    D, P, out = np.zeros((n, n)), np.zeros((4, 3)), np.zeros(4 * n)
    d, p, o = D.ctypes.data, P.ctypes.data, out.ctypes.data
    assert _f("qc_density_on_points", vp, vp, i64, vp, vp)(h, d, 4, p, o) == NODEV
    assert _f("qc_esp_on_points", vp, vp, i64, vp, vp, vp)(h, d, 4, p, o, None) == NODEV
    assert _f("qc_orbitals_on_points", vp, ci, vp, i64, vp, vp)(h, 1, d, 4, p, o) == NODEV
    assert _f("qc_density_on_points", vp, vp, i64, vp, vp)(h, None, 4, p, o) == INV
    assert _f("qc_orbitals_on_points", vp, ci, vp, i64, vp, vp)(h, 0, d, 4, p, o) == INV
    with pytest.raises(q.QcError, match="no CPU fallback"):
        s.density_on_points(D, P)
    s.close()


def test_point_calls_on_a_sharded_handle_are_unsupported():
    import qchem_rs_amd as q
    s = q.System(load_system("water", "STO-3G"))
    s.set_shard(0, 2)
    n, h = s.n, s.handle
    D, P, out = np.zeros((n, n)), np.zeros((4, 3)), np.zeros(4 * n)
    d, p, o = D.ctypes.data, P.ctypes.data, out.ctypes.data
    UNS = q.hf.QC_ERR_UNSUPPORTED
    assert _f("qc_density_on_points", vp, vp, i64, vp, vp)(h, d, 4, p, o) == UNS
    assert _f("qc_esp_on_points", vp, vp, i64, vp, vp, vp)(h, d, 4, p, o, None) == UNS
    assert _f("qc_orbitals_on_points", vp, ci, vp, i64, vp, vp)(h, 1, d, 4, p, o) == UNS
    s.close()


# ---- the command line

def _args(*extra, sub="rhf"):
    return [sub, "-b", data("basis", "STO-3G.json"), "-m", data("mol", "hydrogen.json")] + list(extra)


def test_cli_accepts_cube_and_keeps_the_defaults():
    from qchem_rs_amd import cli
    a = cli.parse_args(_args())
    assert a.cube is None and a.cube_file is None and a.cube_spacing == 0.2 and a.cube_margin == 4.0
    for what in ("density", "esp", "homo", "lumo", "mo:0", "mo:12"):
        assert cli.parse_args(_args("--cube", what, "--cube-file", "x.cube")).cube == what
    a = cli.parse_args(_args("--cube", "spin", "--cube-file", "x.cube", "--cube-spacing", "0.5", "--cube-margin", "3", sub="uhf"))
    assert (a.cube, a.cube_spacing, a.cube_margin) == ("spin", 0.5, 3.0)
    assert cli.cube_what("mo:3", False) == ("mo", 3) and cli.cube_what("spin", False) is None and cli.cube_what("spin", True) == ("spin", None)


@pytest.mark.parametrize("extra,sub", [(("--cube", "charge", "--cube-file", "x.cube"), "rhf"), (("--cube", "density"), "rhf"),
                                       (("--cube", "spin", "--cube-file", "x.cube"), "rhf"), (("--cube", "mo:-1", "--cube-file", "x.cube"), "rhf"),
                                       (("--cube", "mo:x", "--cube-file", "x.cube"), "uhf"), (("--cube-file", "x.cube"), "rhf"),
                                       (("--cube", "esp", "--cube-file", "x.cube", "--cube-spacing", "0"), "rhf"),
                                       (("--cube", "esp", "--cube-file", "x.cube", "--follow"), "uhf")])
def test_cli_rejects_bad_cube_arguments(extra, sub, capsys):
    from qchem_rs_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.parse_args(_args(*extra, sub=sub))
    assert e.value.code == 2
    capsys.readouterr()


def test_cube_file_format(tmp_path):
    """the writer alone: header, atoms, six values per line as %13.5E, a line break after every z run"""
    from qchem_rs_amd import cli
    m = _h2_sto3g()
    origin, shape, pts = cli.cube_grid(m, 1.0, 1.0)
    assert shape == [3, 3, 4] and len(pts) == 36 and np.allclose(pts[1] - pts[0], [0, 0, 1.0]) and np.allclose(pts[4] - pts[0], [0, 1.0, 0])
    val = np.arange(36, dtype=float) - 7.5
    path = str(tmp_path / "t.cube")
    cli.write_cube(path, m, "density", origin, shape, 1.0, val)
    lines = open(path).read().splitlines()
    assert lines[2].split() == ["2", "-1.000000", "-1.000000", "-1.000000"]
    assert [l.split() for l in lines[3:6]] == [["3", "1.000000", "0.000000", "0.000000"], ["3", "0.000000", "1.000000", "0.000000"],
                                               ["4", "0.000000", "0.000000", "1.000000"]]
    assert lines[6].split() == ["1", "1.000000", "0.000000", "0.000000", "0.000000"] and lines[7].split()[4] == "1.400000"
    body = lines[8:]
    assert len(body) == 9 and all(len(l) == 4 * 13 for l in body)               # one line per z run of four values
    assert body[0] == " -7.50000E+00 -6.50000E+00 -5.50000E+00 -4.50000E+00"
    assert np.allclose(np.array(" ".join(body).split(), float), val)
