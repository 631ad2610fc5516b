"""CPU tests of the gradient surface: the new entry points are declared, exported and built; their argument checks run on the host
before any device is touched; without a device they report it; the CLI accepts --gradient on both sub-commands."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, data, load_system

NEW = ("qc_gradient", "qc_scf_gradient", "qc_gradient_timings")


def test_gradient_entry_points_are_declared_listed_and_exported():
    import qchem_rs_amd as q
    header = open(os.path.join(ROOT, "include", "qchem_hip.h")).read()
    declared = set(re.findall(r"\b(qc_[a-z0-9_]+)\s*\(", header))
    L = q.lib()
    for name in NEW:
        assert name in declared, name
        assert name in q.hf.EXPORTS, name
        assert hasattr(L, name), name
    for name in ("restricted_gradient", "unrestricted_gradient"):
        assert hasattr(q, name), name
    ffi = open(os.path.join(ROOT, "bindings", "rust", "qchem-hip", "src", "ffi.rs")).read()
    assert "pub fn qc_gradient(" in ffi and "pub fn qc_scf_gradient(" in ffi


def _call(fn, *args):
    import qchem_rs_amd as q
    vp = ctypes.c_void_p
    f = ctypes.CFUNCTYPE(ctypes.c_int, *([vp] * len(args)))((fn, q.lib()))
    return f(*args)


def _qc_gradient(s, nspin, D, W, terms):
    import qchem_rs_amd as q
    vp = ctypes.c_void_p
    ptr = lambda a: None if a is None else a.ctypes.data_as(vp)
    f = ctypes.CFUNCTYPE(ctypes.c_int, vp, ctypes.c_int, vp, vp, vp)(("qc_gradient", q.lib()))
    return f(s.handle, nspin, ptr(D), ptr(W), ptr(terms))


def test_gradient_argument_errors_are_reported_before_the_device():
    import qchem_rs_amd as q
    s = q.System(load_system("water", "STO-3G"))
    n = s.n
    D, W, t = np.zeros((2, n, n)), np.zeros((n, n)), np.zeros(4 * 9)
    INV = q.hf.QC_ERR_INVALID
    assert _qc_gradient(s, 1, None, W, t) == INV
    assert _qc_gradient(s, 1, D, None, t) == INV
    assert _qc_gradient(s, 1, D, W, None) == INV
    assert _qc_gradient(s, 0, D, W, t) == INV
    assert _qc_gradient(s, 3, D, W, t) == INV
    f = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)(("qc_gradient", q.lib()))
    assert f(None, 1, D.ctypes.data, W.ctypes.data, t.ctypes.data) == INV
    assert _call("qc_scf_gradient", None, t.ctypes.data) == INV
    assert _call("qc_gradient_timings", None, t.ctypes.data) == INV
    assert _call("qc_gradient_timings", s.handle, None) == INV


def test_gradient_without_a_device_returns_no_device():
    import qchem_rs_amd as q
    if q.device_ready():
        pytest.skip("GPU present")
    s = q.System(load_system("water", "STO-3G"))
    n = s.n
    D, W, t = np.zeros((2, n, n)), np.zeros((n, n)), np.zeros(4 * 9)
    assert _qc_gradient(s, 1, D, W, t) == q.hf.QC_ERR_NO_DEVICE
    assert _qc_gradient(s, 2, D, W, t) == q.hf.QC_ERR_NO_DEVICE
    with pytest.raises(q.QcError, match="no CPU fallback"):
        s.gradient(D[0], W)


def test_gradient_on_a_sharded_handle_is_unsupported_without_a_device():
    import qchem_rs_amd as q
    s = q.System(load_system("water", "STO-3G"))
    s.set_shard(0, 2)
    n = s.n
    D, W, t = np.zeros((n, n)), np.zeros((n, n)), np.zeros(4 * 9)
    assert _qc_gradient(s, 1, D, W, t) == q.hf.QC_ERR_UNSUPPORTED


@pytest.mark.parametrize("sub", ["rhf", "uhf"])
def test_cli_accepts_gradient(sub):
    from qchem_rs_amd import cli
    B, M = data("basis", "STO-3G.json"), data("mol", "water.json")
    assert cli.parse_args([sub, "-b", B, "-m", M]).gradient is False
    a = cli.parse_args([sub, "-b", B, "-m", M, "--gradient", "--mp2"])
    assert a.gradient is True and a.mp2 is True


def test_cli_prints_gradient_lines_after_the_references(monkeypatch, capsys):
    import json
    from qchem_rs_amd import cli, hf
    B, M = data("basis", "STO-3G.json"), data("mol", "water.json")
    out = hf.RestrictedHartreeFockOutput([-20.24289, -1.26698, 0.60563], -84.151059, 9.188258, 11)
    g = np.array([[0.0, 0.0, -0.1], [0.0, 0.05, 0.05], [0.0, -0.05, 0.05]])
    monkeypatch.setattr(hf, "_stepped", lambda system, cfg, uhf, after: (out, (None, g)))
    assert cli.main(["rhf", "-b", B, "-m", M, "--gradient", "--json"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[4] == "orbital energies: [-20.243, -1.267, 0.606]"
    z0 = str(load_system("water", "STO-3G").atoms[0].ordinal)
    assert lines[5].split() == ["0", z0, "0.0000000000", "0.0000000000", "-0.1000000000"]
    assert len(lines) == 9 and json.loads(lines[8])["gradient"] == g.tolist()
