"""Host tests of the conductor-like continuum: the cavity surface and its matrix S against the numpy statement
(tests/solvent_reference.py), the properties of S the bounds of the GPU tests rest on, the reference itself on the Born sphere, the bar of
the GPU inverse test on numpy's own inverse, argument errors, the combinations refused without a device, and the command line.

Surfaces: water, ethylene, chloroform and benzene at 1, 2 and 5 points per Angstrom^2 (scale 1.2): M = 43 / 85 / 216, 84 / 150 / 376,
106 / 216 / 537, 107 / 198 / 502.  Measured: positions, areas and S agree with numpy to 0 .. 2e-16 relative; the worst S is benzene at
density 2, lambda_min = 0.0297, cond_2 = 1271; the point-charge form 1 / r_ij with Klamt's diagonal has lambda_min = -11.2 there (and is
indefinite on five of the twelve surfaces), which is why the erf form is used: K = -f S^-1 needs a positive definite S for the device
Cholesky factorisation and for G_pol <= 0.  Born sphere (R = 2 bohr, unit charge): 0.42 % at N = 32, 0.27 % at N = 110 from -f / 2R.
numpy.linalg.inv on the matrices of the GPU inverse test: at most 0.02 of the bar 8 n u cond_2 (margin asked for: 10)."""
import ctypes
import json

import numpy as np
import pytest

from conftest import data, load_system
import solvent_reference as SR

MOLECULES = ("water", "ethylene", "chloroform", "benzene")
DENSITIES = (1.0, 2.0, 5.0)
SURFACES = [(m, d) for m in MOLECULES for d in DENSITIES]
EPS = 78.39
_CASES = {}


def case(mol, density):
    """library surface and S, numpy surface and S - computed once"""
    if (mol, density) not in _CASES:
        import qchem_rs_amd as q
        m = load_system(mol, "STO-3G")
        s = q.System(m)
        s.set_solvent(EPS, density=density)
        P, a, own = s.solvent_surface()
        Pr, ar, ownr = SR.surface(m.atomic_numbers(), m.coordinates(), 1.2, density)
        _CASES[(mol, density)] = dict(P=P, a=a, own=own, Pr=Pr, ar=ar, ownr=ownr, S=s.solvent_matrix(), Sr=SR.s_matrix(Pr, ar), M=s.solvent_points())
        s.close()
    return _CASES[(mol, density)]


@pytest.mark.parametrize("mol,density", SURFACES)
def test_surface_is_the_numpy_rule(mol, density):
    c = case(mol, density)
    assert c["M"] == len(c["ar"]) == len(c["a"]) and np.array_equal(c["own"], c["ownr"])
    dp, da = float(np.abs(c["P"] - c["Pr"]).max()), float(np.abs(c["a"] - c["ar"]).max())
    print(mol, density, "M", c["M"], "max |dP|", dp, "max |da|", da)
    assert dp <= 1e-12 and da <= 1e-12
    if mol == "water":
        assert c["M"] == {1.0: 43, 2.0: 85, 5.0: 216}[density]


@pytest.mark.parametrize("mol,density", SURFACES)
def test_host_matrix_is_the_numpy_matrix(mol, density):
    c = case(mol, density)
    rel = float((np.abs(c["S"] - c["Sr"]) / np.abs(c["Sr"])).max())
    print(mol, density, "max relative |dS|", rel)
    assert rel <= 1e-13 and np.array_equal(c["S"], c["S"].T)


def test_matrix_is_positive_definite_and_well_conditioned_and_the_point_charge_form_is_not():
    negative = 0
    for mol, density in SURFACES:
        c = case(mol, density)
        w = np.linalg.eigvalsh(c["Sr"])
        wp = np.linalg.eigvalsh(SR.s_matrix_point_charges(c["Pr"], c["ar"]))
        print(mol, density, "lambda_min", w[0], "cond_2", w[-1] / w[0], "| 1/r form: lambda_min", wp[0])
        assert w[0] > 0.0 and w[-1] / w[0] < 2000.0
        negative += wp[0] < 0.0
    assert negative >= 1          # the erf form is used because this one cannot be factored and does not bound G_pol


def test_reference_reproduces_the_born_sphere():
    for N in (32, 110, 300):
        g, exact = SR.born(2.0, N, EPS)
        print("N", N, "G_pol", g, "-f/2R", exact, "relative", abs(g - exact) / abs(exact))
        assert abs(g - exact) <= 5e-3 * abs(exact)
    g, exact = SR.born(2.0, 110, EPS, x=0.5)
    assert abs(g - exact) <= 5e-3 * abs(exact) and abs(exact + (EPS - 1.0) / (EPS + 0.5) / 4.0) < 1e-15


@pytest.mark.parametrize("n", SR.INVERSE_SIZES)
def test_numpy_inverse_meets_the_bar_of_the_gpu_inverse_test_with_a_margin_of_ten(n):
    for k in SR.INVERSE_DECADES:
        A = SR.spd_matrix(n, k)
        w = np.linalg.eigvalsh(A)
        cond = w[-1] / w[0]
        err = float(np.abs(A @ np.linalg.inv(A) - np.eye(n)).max())
        print("n", n, "k", k, "cond_2", cond, "max |A inv(A) - I|", err, "bar", SR.inverse_bar(n, cond))
        assert np.array_equal(A, A.T) and w[0] > 0.0 and (n == 1 or abs(cond / 10.0 ** k - 1.0) < 1e-10)
        assert err <= SR.inverse_bar(n, cond) / 10.0


# ---- the C surface without a device
vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def _f(name, *argtypes, restype=ctypes.c_int):
    import qchem_rs_amd as q
    fn = getattr(ctypes.CDLL(q.hf.LIB_PATH), name)
    fn.argtypes, fn.restype = list(argtypes), restype
    return fn


def _cfg(eps=EPS, x=0.0, scale=0.0, density=1.0):
    import qchem_rs_amd as q
    return q.hf._Solvent(eps, x, scale, density)


def test_exports_and_struct_sizes():
    import qchem_rs_amd as q
    L = q.lib()
    for name in ("qc_spd_inverse", "qc_set_solvent", "qc_solvent_surface", "qc_solvent_matrix", "qc_solvent_matrix_gpu", "qc_solvent_response",
                 "qc_scf_solvent", "qc_solvent_last", "qc_solvent_timings"):
        assert hasattr(L, name) and name in q.hf.EXPORTS
    assert ctypes.sizeof(q.hf._Solvent) == 32 and ctypes.sizeof(q.hf._SolventEnergy) == 32


def test_argument_errors_of_every_entry_point():
    import qchem_rs_amd as q
    INV, OK = q.hf.QC_ERR_INVALID, q.hf.QC_OK
    s = q.System(load_system("water", "STO-3G"))
    h, n = s.handle, s.n
    set_solvent = _f("qc_set_solvent", vp, vp, vp)
    surface = _f("qc_solvent_surface", vp, i64, vp, vp, vp, restype=i64)
    buf = np.zeros(max(n * n, 64))
    b = buf.ctypes.data
    # nothing set yet: the calls that need a cavity say so
    assert surface(h, 0, None, None, None) == INV
    assert _f("qc_solvent_matrix", vp, vp)(h, b) == INV
    assert _f("qc_solvent_matrix_gpu", vp, vp, vp)(h, b, None) == INV
    assert _f("qc_solvent_response", vp, vp, vp, vp, vp)(h, b, None, None, b) == INV
    assert _f("qc_solvent_last", vp, vp)(h, b) == INV and _f("qc_solvent_timings", vp, vp)(h, b) == INV
    assert _f("qc_scf_solvent", vp, vp, vp)(None, b, None) == INV
    # bad configurations leave the handle as it was
    assert set_solvent(None, ctypes.byref(_cfg()), None) == INV
    for bad in (_cfg(eps=1.0), _cfg(eps=0.5), _cfg(eps=float("nan")), _cfg(eps=float("inf")), _cfg(x=-0.1), _cfg(x=float("nan")),
                _cfg(scale=-1.0), _cfg(scale=float("inf")), _cfg(density=-1.0), _cfg(density=float("nan"))):
        assert set_solvent(h, ctypes.byref(bad), None) == INV
    for radii in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [float("nan"), 1.0, 1.0]):
        r = np.array(radii)
        assert set_solvent(h, ctypes.byref(_cfg()), r.ctypes.data) == INV
    assert surface(h, 0, None, None, None) == INV                            # still no cavity
    # spheres that overlap, and one that lies inside another (it keeps no point; the outer one keeps all of its own)
    m2 = q.MolecularSystem.from_atoms([q.Atom(1, [0.0, 0.0, 0.0]), q.Atom(1, [0.0, 0.0, 0.1])], q.BasisSet.load(data("basis", "STO-3G.json")))
    s2 = q.System(m2)
    assert set_solvent(s2.handle, ctypes.byref(_cfg()), None) == OK       # overlapping equal spheres keep their outer caps
    r = np.array([0.5, 5.0])
    assert set_solvent(s2.handle, ctypes.byref(_cfg()), r.ctypes.data) == OK and surface(s2.handle, 0, None, None, None) > 0
    s2.close()
    # more than 16384 elements
    assert set_solvent(h, ctypes.byref(_cfg(density=400.0)), None) == q.hf.QC_ERR_UNSUPPORTED
    assert surface(h, 0, None, None, None) == INV
    # a good one, custom radii, then the null arguments of the calls that now have a cavity
    r = np.array([3.0, 2.0, 2.0])
    assert set_solvent(h, ctypes.byref(_cfg()), r.ctypes.data) == OK
    P, a, own = s.solvent_surface()
    Pr, ar, ownr = SR.surface(s.mol.atomic_numbers(), s.mol.coordinates(), 1.2, 1.0, radii=r)
    assert len(a) == len(ar) and np.array_equal(own, ownr) and np.abs(P - Pr).max() <= 1e-12 and np.abs(a - ar).max() <= 1e-12
    M = len(a)
    small = np.full(3, 7.0)
    assert surface(h, M - 1, small.ctypes.data, None, None) == M and np.all(small == 7.0)     # too small a capacity: only M comes back
    assert _f("qc_solvent_matrix", vp, vp)(h, None) == INV
    assert _f("qc_solvent_response", vp, vp, vp, vp, vp)(h, None, None, None, b) == INV
    assert _f("qc_solvent_response", vp, vp, vp, vp, vp)(h, b, None, None, None) == INV
    assert _f("qc_solvent_last", vp, vp)(h, b) == INV                        # no run yet
    assert _f("qc_solvent_timings", vp, vp)(h, None) == INV
    spd = _f("qc_spd_inverse", vp, ci, vp, vp)
    assert spd(None, 2, b, b) == INV and spd(h, 0, b, b) == INV and spd(h, 2, None, b) == INV and spd(h, 2, b, None) == INV
    with pytest.raises(q.QcError):
        s.set_solvent(EPS, model="pcm")
    with pytest.raises(q.QcError):
        s.set_solvent(EPS, radii=[1.0, 2.0])
    s.set_solvent(None)
    assert surface(h, 0, None, None, None) == INV
    s.close()


def test_models_and_defaults():
    import qchem_rs_amd as q
    m = load_system("water", "STO-3G")
    s = q.System(m)
    s.set_solvent(EPS)                                                       # scale 1.2, 5 per A^2
    assert s.solvent_points() == 216
    s.set_solvent(EPS, model="cosmo", scale=1.4, density=2.0)
    P, a, own = s.solvent_surface()
    Pr, ar, ownr = SR.surface(m.atomic_numbers(), m.coordinates(), 1.4, 2.0)
    assert len(a) == len(ar) and np.abs(P - Pr).max() <= 1e-12 and np.array_equal(own, ownr)
    assert q.hf.SOLVENT_MODELS == {"cpcm": 0.0, "cosmo": 0.5}
    out = q.RestrictedHartreeFockOutput([], -1.0, 0.25, 3, {}, 0.125, -0.0625)
    assert out.solvent_nuclear_energy == -0.0625 and out.total_energy() == -1.0 + 0.25 + 0.125 - 0.0625
    out = q.UnrestrictedHartreeFockOutput([], [], -1.0, 0.25, 3)
    assert out.solvent_nuclear_energy == 0.0 and out.total_energy() == -0.75
    s.close()


def test_combinations_refused_before_the_device_is_touched():
    """a solvent with a shard, the stored-tensor mode or point charges: QC_ERR_UNSUPPORTED from the begin calls and the one-shot drivers,
    with or without a device"""
    import qchem_rs_amd as q
    UNS = q.hf.QC_ERR_UNSUPPORTED
    m = load_system("water", "STO-3G")
    L = q.lib()

    def attempts(s):
        st = ctypes.c_void_p()
        D = np.zeros((s.n, s.n))
        w = np.zeros(s.n)
        out = q.hf._Output()
        out.orbital_energies = w.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        out.orbital_energies_beta = w.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        cfg = q.hf._Config(10, 1e-6, 0, 0)
        return [L.qc_scf_begin_rhf(s.handle, ctypes.byref(st)), L.qc_scf_begin_uhf(s.handle, 0, 0, ctypes.byref(st)),
                L.qc_scf_begin_rhf_from(s.handle, D.ctypes.data, ctypes.byref(st)),
                L.qc_scf_begin_uhf_from(s.handle, 5, 5, D.ctypes.data, D.ctypes.data, ctypes.byref(st)),
                L.qc_scf_rhf(s.handle, ctypes.byref(cfg), ctypes.byref(out)), L.qc_scf_uhf(s.handle, ctypes.byref(cfg), ctypes.byref(out))]

    for prepare in (lambda s: s.set_shard(0, 2), lambda s: s.set_fock_mode("stored"),
                    lambda s: s.set_point_charges(np.array([[0.0, 0.0, 6.0]]), np.array([0.5]))):
        s = q.System(m)
        s.set_solvent(EPS, density=1.0)
        prepare(s)
        assert attempts(s) == [UNS] * 6
        s.close()
    s = q.System(m)
    s.set_solvent(EPS, density=1.0)
    s.set_shard(0, 2)
    D, e = np.zeros((s.n, s.n)), np.zeros(2)
    assert _f("qc_solvent_response", vp, vp, vp, vp, vp)(s.handle, D.ctypes.data, None, None, e.ctypes.data) == UNS
    s.close()


def test_compute_calls_without_a_device_return_no_device():
    import qchem_rs_amd as q
    if q.device_ready():
        pytest.skip("GPU present")
    NODEV = q.hf.QC_ERR_NO_DEVICE
    s = q.System(load_system("water", "STO-3G"))
    s.set_solvent(EPS, density=1.0)
    M, n, h = s.solvent_points(), s.n, s.handle
    A, B, D, e = np.eye(4), np.zeros((4, 4)), np.zeros((n, n)), np.zeros(2)
    Sm = np.zeros((M, M))
    assert _f("qc_spd_inverse", vp, ci, vp, vp)(h, 4, A.ctypes.data, B.ctypes.data) == NODEV
    assert _f("qc_solvent_matrix_gpu", vp, vp, vp)(h, Sm.ctypes.data, None) == NODEV
    assert _f("qc_solvent_matrix_gpu", vp, vp, vp)(h, None, Sm.ctypes.data) == NODEV
    assert _f("qc_solvent_response", vp, vp, vp, vp, vp)(h, D.ctypes.data, None, None, e.ctypes.data) == NODEV
    st = ctypes.c_void_p()
    assert q.lib().qc_scf_begin_rhf(h, ctypes.byref(st)) == NODEV
    with pytest.raises(q.QcError, match="no CPU fallback"):
        s.solvent_response(D)
    with pytest.raises(q.QcError, match="no CPU fallback"):
        s.spd_inverse(A)
    assert s.solvent_matrix().shape == (M, M)                                # the host statement needs no device
    s.close()


# ---- the command line

def _args(*extra, sub="rhf"):
    return [sub, "-b", data("basis", "STO-3G.json"), "-m", data("mol", "water.json")] + list(extra)


def test_cli_flags_parse_and_reject():
    from qchem_rs_amd import cli
    for sub in ("rhf", "uhf"):
        a = cli.parse_args(_args(sub=sub))
        assert a.solvent is None and a.solvent_model == "cpcm" and a.solvent_density == 0.0
        a = cli.parse_args(_args("--solvent", "78.39", "--solvent-model", "cosmo", "--solvent-density", "2", "--mp2", "--dipole", sub=sub))
        assert a.solvent == 78.39 and a.solvent_model == "cosmo" and a.solvent_density == 2.0
        for bad in (["--solvent", "1.0"], ["--solvent", "0.5"], ["--solvent", "nan"], ["--solvent", "inf"], ["--solvent", "80", "--solvent-density", "-1"],
                    ["--solvent", "80", "--solvent-model", "pcm"], ["--solvent-model", "cosmo"], ["--solvent-density", "2"],
                    ["--solvent", "80", "--point-charges", "x.json"], ["--solvent", "80", "--gradient"], ["--solvent", "80", "--stability"],
                    ["--solvent", "80", "--follow"], ["--solvent", "80", "--polarizability"]):
            with pytest.raises(SystemExit):
                cli.parse_args(_args(*bad, sub=sub))
    for bad in (["--solvent", "80", "--cis", "2"], ["--solvent", "80", "--tdhf", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_args(_args(*bad))


def test_cli_printed_lines_with_a_stubbed_driver(monkeypatch, capsys):
    from qchem_rs_amd import cli, hf
    sv = hf.SolventOutput(0.123456789, -0.133456789, -3.5e-4, 85)
    seen = {}

    def rhf(system, cfg):
        seen["M"] = system.solvent_points()
        system.last_solvent = sv
        return hf.RestrictedHartreeFockOutput([-20.25, -1.25, 0.5], -84.0, 9.25, 11, {}, 0.0, sv.nuclear)

    monkeypatch.setattr(hf, "restricted_hartree_fock", rhf)
    assert cli.main(_args("--solvent", "78.39", "--solvent-density", "2", "--json")) == 0
    lines = capsys.readouterr().out.splitlines()
    assert seen["M"] == 85
    assert lines[0] == "solvent: cpcm, epsilon %s, surface elements: 85" % cli.fmt_f(78.39)
    assert lines[2] == "electronic energy: " + cli.fmt_f(-84.0) and lines[3] == "nuclear repulsion energy: " + cli.fmt_f(9.25)
    assert lines[4] == "hartree fock energy: " + cli.fmt_f(-84.0 + 9.25 + sv.nuclear)
    assert lines[6] == "solvent 1/2 q.v: nuclei %s, electrons %s, total %s" % (cli.fmt_f(sv.nuclear), cli.fmt_f(sv.electronic), cli.fmt_f(sv.nuclear + sv.electronic))
    assert lines[7] == "solvent surface charge: " + cli.fmt_f(sv.total_charge)
    doc = json.loads(lines[8])
    assert len(lines) == 9 and doc["total_energy"] == -84.0 + 9.25 + sv.nuclear
    assert doc["solvent"] == {"model": "cpcm", "epsilon": 78.39, "points": 85, "nuclear_energy": sv.nuclear, "electronic_energy": sv.electronic,
                              "polarization_energy": sv.nuclear + sv.electronic, "total_charge": sv.total_charge}

    def uhf(system, cfg):
        system.last_solvent = sv
        return hf.UnrestrictedHartreeFockOutput([-20.25], [-20.5], -84.0, 9.25, 12, {}, 0.0, sv.nuclear)

    monkeypatch.setattr(hf, "unrestricted_hartree_fock", uhf)
    assert cli.main(_args("--solvent", "78.39", "--solvent-model", "cosmo", "--solvent-density", "1", sub="uhf")) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "solvent: cosmo, epsilon %s, surface elements: 43" % cli.fmt_f(78.39)
    assert lines[4] == "hartree fock energy: " + cli.fmt_f(-84.0 + 9.25 + sv.nuclear)
    assert lines[7].startswith("solvent 1/2 q.v: nuclei ") and lines[8] == "solvent surface charge: " + cli.fmt_f(sv.total_charge) and len(lines) == 9
    # without the flag nothing of it is printed
    monkeypatch.setattr(hf, "restricted_hartree_fock", lambda system, cfg: hf.RestrictedHartreeFockOutput([-20.25], -84.0, 9.25, 11))
    assert cli.main(_args("--json")) == 0
    out = capsys.readouterr().out
    assert "solvent" not in out
