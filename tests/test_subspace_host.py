"""The host numerics of the reduced-space solvers (qchem-rs_amd/csrc/qc_subspace_host.h) on the CPU: host_sym_eig, host_lu_solve,
tdhf_reduced and qc_orthonormalize_row, driven through the stand-alone program tests/host/subspace_host_main.cpp, which is built here with
the system C++ compiler and -fsanitize=address,undefined.  Nothing is loaded into Python; a sanitizer report fails the run (exit status).

Reference: numpy in float64.  Every bound has the backward-error form K m u |A| (u = 2^-53; for the solves times the 2-norm condition
number numpy reports), with K four times the worst value measured over the seeds listed here with g++ and glibc on x86-64 - the
headroom is for another compiler or libm.  Measured worst values (error / (m u scale)):
  host_sym_eig   |A v - w v| 2.38    |V V^T - 1| 2.86    |w - w_numpy| 2.44      (the same figures at both stop ratios: the sweeps converge
                 quadratically, and the sweep that passes 1e-27 lands below the rounding floor as well)
  host_lu_solve  |x - x_numpy| / (cond |x|) 0.31
  tdhf_reduced   |w^2 - eig(M- M+)| / (|M-| |M+|) 3.79      |L~ . R~ - 1| 2.0
  qc_orthonormalize_row   |Z Z^T - 1| 0.4      |Z - Z_numpy| 0.2
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
SEEDS = (0, 1, 2)
K = {("eig", 1e-32, "res"): 4 * 2.38, ("eig", 1e-32, "orth"): 4 * 2.86, ("eig", 1e-32, "w"): 4 * 2.44,
     ("eig", 1e-27, "res"): 4 * 2.38, ("eig", 1e-27, "orth"): 4 * 2.86, ("eig", 1e-27, "w"): 4 * 2.44,
     "lu": 4 * 0.31, "tdhf_w2": 4 * 3.79, "tdhf_lr": 4 * 2.0, "gs_orth": 4 * 0.4, "gs_numpy": 4 * 0.2}
_worst = {}


def ratio(key, value, scale):
    """value / scale, remembered per bound (printed at the end of the module: the figures of the docstring)"""
    r = float(value) / float(scale)
    _worst[key] = max(_worst.get(key, 0.0), r)
    return r


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = tmp_path_factory.mktemp("subspace_host") / "subspace_host_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "qchem-rs_amd", "csrc"), os.path.join(ROOT, "tests", "host", "subspace_host_main.cpp"), "-o", str(exe)],
                   check=True, timeout=300)
    yield str(exe)
    print("worst error / (m u scale) per bound:", {str(k): round(v, 4) for k, v in _worst.items()})


def run(prog, tmp_path, op, *parts):
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([np.asarray(p, np.float64).ravel() for p in parts]).tofile(fin)
    p = subprocess.run([prog, op, str(fin), str(fout)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return np.fromfile(fout, np.float64)


def sym(seed, m):
    A = np.random.default_rng(seed).standard_normal((m, m))
    return 0.5 * (A + A.T)


def eig_inputs(m):
    out = [("seed%d" % s, sym(s, m)) for s in SEEDS]
    out.append(("diagonal", np.diag(np.arange(m, 0, -1.0) - 0.5 * m)))
    if m >= 2:
        Q = np.linalg.qr(np.random.default_rng(7).standard_normal((m, m)))[0]
        w = np.linspace(-1.0, 2.0, m)
        w[1] = w[0]
        out.append(("degenerate pair", (Q * w) @ Q.T))
    return out


@pytest.mark.parametrize("stop", [1e-32, 1e-27])
@pytest.mark.parametrize("m", [1, 2, 7, 40])
def test_host_sym_eig(prog, tmp_path, m, stop):
    for name, A in eig_inputs(m):
        A = 0.5 * (A + A.T)
        out = run(prog, tmp_path, "eig", [m, stop], A)
        w, V = out[:m], out[m:].reshape(m, m)
        norm = max(np.linalg.norm(A, 2), 1e-300)
        res = max(np.linalg.norm(A @ V[k] - w[k] * V[k]) for k in range(m))
        orth = np.abs(V @ V.T - np.eye(m)).max()
        dw = np.abs(w - np.linalg.eigvalsh(A)).max()
        r = (ratio(("eig", stop, "res"), res, m * U * norm), ratio(("eig", stop, "orth"), orth, m * U), ratio(("eig", stop, "w"), dw, m * U * norm))
        print("eig", m, stop, name, "res, orth, w over m u |A|:", r)
        assert np.all(np.diff(w) >= 0)
        assert r[0] <= K[("eig", stop, "res")] and r[1] <= K[("eig", stop, "orth")] and r[2] <= K[("eig", stop, "w")]


@pytest.mark.parametrize("m", [1, 3, 40])
def test_host_lu_solve(prog, tmp_path, m):
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        A, b = rng.standard_normal((m, m)), rng.standard_normal((3, m))
        if m > 1:
            A[0, 0] = 0.0                                   # the first pivot has to come from another row
        out = run(prog, tmp_path, "lu", [m, 3], A, b)
        x, x_ref = out[1:].reshape(3, m), np.linalg.solve(A, b.T).T
        r = ratio("lu", np.abs(x - x_ref).max(), m * U * np.linalg.cond(A) * np.abs(x_ref).max())
        print("lu", m, seed, "cond", np.linalg.cond(A), "|x - x_numpy| over m u cond |x|:", r)
        assert out[0] == 1.0 and r <= K["lu"]
    # exactly singular: a zero matrix of order 1, otherwise two equal rows (the elimination leaves an exact zero row)
    S = np.zeros((1, 1)) if m == 1 else np.random.default_rng(3).standard_normal((m, m))
    if m > 1:
        S[m - 1] = S[0]
    assert run(prog, tmp_path, "lu", [m, 3], S, np.ones((3, m)))[0] == 0.0


def spd(seed, m):
    Q = np.linalg.qr(np.random.default_rng(seed).standard_normal((m, m)))[0]
    return (Q * np.random.default_rng(seed + 100).uniform(0.5, 3.0, m)) @ Q.T


@pytest.mark.parametrize("m", [2, 6, 40])
def test_tdhf_reduced(prog, tmp_path, m):
    nroots = min(m, 8)
    for seed in SEEDS:
        Mp, Mm = spd(seed, m), spd(seed + 10, m)
        Mp, Mm = 0.5 * (Mp + Mp.T), 0.5 * (Mm + Mm.T)
        out = run(prog, tmp_path, "tdhf", [m, nroots], Mp, Mm)
        omega, Rt, Lt = out[1:1 + nroots], out[1 + nroots:1 + nroots + nroots * m].reshape(nroots, m), out[1 + nroots + nroots * m:].reshape(nroots, m)
        w2 = np.sort(np.linalg.eigvals(Mm @ Mp).real)[:nroots]
        r = (ratio("tdhf_w2", np.abs(omega ** 2 - w2).max(), m * U * np.linalg.norm(Mm, 2) * np.linalg.norm(Mp, 2)),
             ratio("tdhf_lr", np.abs(np.einsum("ki,ki->k", Lt, Rt) - 1.0).max(), m * U))
        print("tdhf", m, seed, "w^2, L.R over m u scale:", r)
        assert out[0] == 1.0 and np.all(np.diff(omega) >= 0)
        assert r[0] <= K["tdhf_w2"] and r[1] <= K["tdhf_lr"]
    Mm = spd(0, m)
    Mm -= 2.0 * np.linalg.eigvalsh(Mm)[0] * np.eye(m)          # the lowest eigenvalue changes sign: indefinite
    assert run(prog, tmp_path, "tdhf", [m, nroots], spd(1, m), 0.5 * (Mm + Mm.T))[0] == 0.0


def numpy_rows(src, m, ld):
    """the same two-pass modified Gram-Schmidt with the QC_STAB_KEEP rule"""
    Z, kept = [], []
    for s in src:
        z = s.copy()
        before = z @ z
        for _ in range(2):
            for r in Z:
                z = z - (z @ r) * r
        after = z @ z
        kept.append(bool(after > 1e-4 * 1e-4 * before))
        if kept[-1]:
            Z.append(z / np.sqrt(after))
    return np.array(Z), kept


@pytest.mark.parametrize("m,ld", [(5, 5), (24, 40), (40, 40)])
def test_qc_orthonormalize_row(prog, tmp_path, m, ld):
    for seed in SEEDS:
        rng = np.random.default_rng(seed)
        src = rng.standard_normal((4, m))
        src = np.vstack([src[:3], 0.3 * src[0] - 2.0 * src[2], src[3:]])        # the fourth is a combination of earlier ones
        out = run(prog, tmp_path, "gs", [ld, m, len(src)], src)
        k, rec = int(out[0]), out[1:].reshape(len(src), 1 + ld)
        kept, rows = rec[:, 0] == 1.0, rec[:, 1:]
        Z_ref, kept_ref = numpy_rows(src, m, ld)
        assert k == 4 and kept.tolist() == kept_ref == [True, True, True, False, True]
        assert not rows[3].any() and not rows[:, m:].any()                      # the dropped row is zeroed; nothing beyond m is touched
        Z = rows[kept][:, :m]
        r = (ratio("gs_orth", np.abs(Z @ Z.T - np.eye(k)).max(), m * U), ratio("gs_numpy", np.abs(Z - Z_ref).max(), m * U))
        print("gs", m, ld, seed, "orth, numpy over m u:", r)
        assert r[0] <= K["gs_orth"] and r[1] <= K["gs_numpy"]
