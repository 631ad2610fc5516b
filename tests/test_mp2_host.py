"""CPU tests of the MP2 surface: the three new entry points are declared, exported and built; their argument checks run on the host
before any device is touched; the CLI accepts --mp2 / --frozen-core on both sub-commands."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, data, load_system

NEW = ("qc_scf_coefficients", "qc_scf_mp2", "qc_mp2")


def test_mp2_entry_points_are_declared_listed_and_exported():
    import qchem_rs_amd as q
    header = open(os.path.join(ROOT, "include", "qchem_hip.h")).read()
    declared = set(re.findall(r"\b(qc_[a-z0-9_]+)\s*\(", header))
    L = q.lib()
    for name in NEW:
        assert name in declared, name
        assert name in q.hf.EXPORTS, name
        assert hasattr(L, name), name
    assert "qc_mp2_output" in header


def _orbitals(n, nocc, nspin=1, seed=0):
    rng = np.random.default_rng(seed)
    C = np.concatenate([np.linalg.qr(rng.standard_normal((n, n)))[0] for _ in range(nspin)])
    eps = np.concatenate([np.r_[np.linspace(-2.0, -0.5, n_o), np.linspace(0.3, 2.0, n - n_o)] for n_o in nocc])
    return np.ascontiguousarray(C), np.ascontiguousarray(eps)


def _qc_mp2(s, nspin, C, eps, nocc, n_frozen, out=True):
    import qchem_rs_amd as q
    o = q.hf._Mp2Output()
    vp = ctypes.c_void_p
    L = q.lib()
    ptr = lambda a: None if a is None else a.ctypes.data_as(vp)
    f = ctypes.CFUNCTYPE(ctypes.c_int, vp, ctypes.c_int, vp, vp, vp, ctypes.c_int32, vp)(("qc_mp2", L))
    return f(s.handle, nspin, ptr(C), ptr(eps), ptr(None if nocc is None else np.asarray(nocc, np.int32)), n_frozen,
             ctypes.cast(ctypes.byref(o), vp) if out else None)


def test_mp2_argument_errors_are_reported_before_the_device():
    import qchem_rs_amd as q
    s = q.System(load_system("water", "STO-3G"))
    n = s.n
    C, eps = _orbitals(n, [5])
    INV = q.hf.QC_ERR_INVALID
    assert _qc_mp2(s, 1, C, eps, [5], -1) == INV                    # n_frozen < 0
    assert _qc_mp2(s, 1, C, eps, [5], 6) == INV                     # n_frozen > nocc
    assert _qc_mp2(s, 1, None, eps, [5], 0) == INV                  # null pointers
    assert _qc_mp2(s, 1, C, None, [5], 0) == INV
    assert _qc_mp2(s, 1, C, eps, None, 0) == INV
    assert _qc_mp2(s, 1, C, eps, [5], 0, out=False) == INV
    assert _qc_mp2(s, 3, C, eps, [5], 0) == INV                     # nspin
    assert _qc_mp2(s, 1, C, eps, [8], 0) == INV                     # nocc > n
    bad = eps.copy(); bad[4] = bad[5]                                # highest occupied = lowest virtual: a zero denominator
    assert _qc_mp2(s, 1, C, bad, [5], 0) == INV
    bad = eps.copy(); bad[0] = 1.0                                   # an occupied orbital above the virtuals
    assert _qc_mp2(s, 1, C, bad, [5], 0) == INV
    assert _qc_mp2(s, 1, C, bad, [5], 1) != INV                     # ... but frozen: it takes no part
    C2, eps2 = _orbitals(n, [5, 4], nspin=2)
    assert _qc_mp2(s, 2, C2, eps2, [5, 4], 5) == INV                # n_frozen > min(n_alpha, n_beta)
    bad = eps2.copy(); bad[n + 3] = 5.0                              # beta occupied above the beta virtuals
    assert _qc_mp2(s, 2, C2, bad, [5, 4], 0) == INV


def test_mp2_without_a_device_returns_no_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import qchem_rs_amd as q
    s = q.System(load_system("water", "STO-3G"))
    C, eps = _orbitals(s.n, [5])
    assert _qc_mp2(s, 1, C, eps, [5], 0) == q.hf.QC_ERR_NO_DEVICE
    C2, eps2 = _orbitals(s.n, [5, 0], nspin=2)                      # an empty beta block is no error either
    assert _qc_mp2(s, 2, C2, eps2, [5, 0], 0) == q.hf.QC_ERR_NO_DEVICE
    with pytest.raises(q.QcError, match="no CPU fallback"):
        s.mp2(C, eps, 5)


def test_mp2_on_a_sharded_handle_is_unsupported_without_a_device():
    import qchem_rs_amd as q
    s = q.System(load_system("water", "STO-3G"))
    s.set_shard(0, 2)
    C, eps = _orbitals(s.n, [5])
    assert _qc_mp2(s, 1, C, eps, [5], 0) == q.hf.QC_ERR_UNSUPPORTED


def _cli():
    import qchem_rs_amd  # noqa: F401
    from qchem_rs_amd import cli
    return cli


@pytest.mark.parametrize("sub", ["rhf", "uhf"])
def test_cli_accepts_mp2_and_frozen_core(sub):
    cli = _cli()
    B, M = data("basis", "STO-3G.json"), data("mol", "water.json")
    a = cli.parse_args([sub, "-b", B, "-m", M])
    assert a.mp2 is False and a.frozen_core is None
    a = cli.parse_args([sub, "-b", B, "-m", M, "--mp2"])
    assert a.mp2 is True and a.frozen_core is None
    a = cli.parse_args([sub, "-b", B, "-m", M, "--mp2", "--frozen-core", "1"])
    assert a.mp2 is True and a.frozen_core == 1
    with pytest.raises(SystemExit):
        cli.parse_args([sub, "-b", B, "-m", M, "--frozen-core", "1"])
    with pytest.raises(SystemExit):
        cli.main([sub, "-b", B, "-m", M, "--frozen-core", "1"])


def test_cli_prints_mp2_lines_after_the_references(monkeypatch, capsys):
    import json
    cli = _cli()
    from qchem_rs_amd import hf
    B, M = data("basis", "STO-3G.json"), data("mol", "water.json")
    out = hf.RestrictedHartreeFockOutput([-20.24289, -1.26698, 0.60563], -84.151059, 9.188258, 11)
    mp2 = hf.Mp2Output(-0.03, -0.01, -0.04, 1.0, 2.0, 3.0, 1)
    seen = {}
    monkeypatch.setattr(hf, "restricted_mp2", lambda system, cfg, n_frozen: seen.update(nf=n_frozen, eps=cfg.epsilon) or (out, mp2))
    assert cli.main(["rhf", "-b", B, "-m", M, "--mp2", "--frozen-core", "1", "--epsilon", "1e-10", "--json"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert seen == {"nf": 1, "eps": 1e-10}
    assert lines[1:5] == ["electronic energy: -84.151", "nuclear repulsion energy: 9.188", "hartree fock energy: -74.963",
                          "orbital energies: [-20.243, -1.267, 0.606]"]
    assert lines[5:7] == ["mp2 correlation energy: -0.040", "mp2 total energy: -75.003"]
    doc = json.loads(lines[7])["mp2"]
    assert doc["e_os"] == -0.03 and doc["e_ss"] == -0.01 and doc["e_corr"] == -0.04 and doc["n_frozen"] == 1
    assert abs(doc["e_total"] - (out.total_energy() - 0.04)) < 1e-15 and doc["timings_ms"]["transform"] == 2.0
