"""Every output of the reduced-space solvers (stability, CPHF polarizability, CIS / TDHF) and of MP2 as hex, for ONE library.

    QCHEM_HIP_LIB=<parent.so> python tools/subspace_ab.py > parent.txt
    QCHEM_HIP_LIB=<change.so> python tools/subspace_ab.py > change.txt      (a process of its own), then  cmp parent.txt change.txt

One line per value: `<run> <name> <count or shape> <hex of the bytes>`; integers (rounds, builds, products, statuses) in decimal.  Two
libraries that compute the same thing print the same text.  Times are not printed.  --only stability|polarizability|excitations|mp2.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import qchem_rs_amd as q  # noqa: E402


def mol(name):
    m, basis = name.split("/")
    if m.startswith("h2@"):
        b = q.BasisSet.load(os.path.join(ROOT, "data", "basis", basis + ".json"))
        return q.MolecularSystem.from_atoms([q.Atom(1, [0.0, 0.0, 0.0]), q.Atom(1, [0.0, 0.0, float(m[3:])])], b)
    return q.MolecularSystem.load(os.path.join(ROOT, "data", "mol", m + ".json"), q.BasisSet.load(os.path.join(ROOT, "data", "basis", basis + ".json")))


def converged(m, uhf=False, na=0, nb=0, eps=1e-10, density=None):
    s = q.System(m)
    s.set_schwarz(0.0)
    st = q.ScfStepper(s, uhf=uhf, n_alpha=na, n_beta=nb, density=density) if density is not None else q.ScfStepper(s, uhf=uhf, n_alpha=na, n_beta=nb)
    for _ in range(2000):
        _, rms = st.iterate()
        if (rms / 2.0 if uhf else rms) < eps:
            return s, st
    raise SystemExit("subspace_ab: a state did not converge")


def put(run, name, x):
    if isinstance(x, (bool, int, np.integer)):
        print(run, name, int(x))
        return
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    print(run, name, "x".join(map(str, a.shape)) or "1", a.tobytes().hex())


def stability():
    # the cases of test_a_call_is_bitwise_reproducible, benzene/STO-3G with 8 roots (more builds than the subspace holds rows: it
    # collapses) and water/6-31G (dim 40: the whole-space start)
    for name, uhf, na, nb, kind, nroots in (("water/cc-pVDZ", False, 0, 0, 1, 3), ("oxygen/cc-pVDZ", True, 9, 7, 0, 4), ("benzene/STO-3G", False, 0, 0, 0, 8),
                                            ("water/6-31G", False, 0, 0, 0, 8)):
        s, st = converged(mol(name), uhf, na, nb)
        r = st.stability(kind=kind, nroots=nroots, tol=1e-7, vectors=True)
        run = "stability:%s:k%d" % (name, kind)
        put(run, "eigenvalues", r.eigenvalues); put(run, "residuals", r.residuals); put(run, "vectors", r.vectors)
        put(run, "iterations", r.iterations); put(run, "builds", r.builds); put(run, "converged", r.converged)
        st.close(); s.close()


def polarizability():
    def dump(run, st):
        p = st.polarizability(tol=1e-7, response=True)
        put(run, "alpha", p.alpha); put(run, "residuals", p.residuals); put(run, "response", p.response); put(run, "asymmetry", p.asymmetry)
        put(run, "iterations", p.iterations); put(run, "builds", p.builds); put(run, "converged", p.converged)

    # (benzene/6-31G takes more builds than the subspace holds rows: the collapse of the CPHF loop)
    for name, uhf, na, nb in (("h2@1.4/6-31G", False, 0, 0), ("water/cc-pVDZ", False, 0, 0), ("water/cc-pVDZ", True, 5, 5), ("benzene/STO-3G", False, 0, 0),
                              ("benzene/6-31G", False, 0, 0)):
        s, st = converged(mol(name), uhf, na, nb)
        dump("polarizability:%s:%s" % (name, "uhf" if uhf else "rhf"), st)
        st.close(); s.close()
    # the H atom: an empty beta block, begun from the lowest eigenvector of the core Hamiltonian (self-consistent for one electron)
    import scipy.linalg as sl
    m = mol("h_atom/6-311++G_st_st")
    h = q.System(m)
    _, Cm = sl.eigh(h.kinetic() + h.nuclear(), h.overlap())
    h.close()
    Da = np.outer(Cm[:, 0], Cm[:, 0])
    s = q.System(m)
    s.set_schwarz(0.0)
    st = q.ScfStepper(s, uhf=True, n_alpha=1, n_beta=0, density=(Da, np.zeros_like(Da)))
    st.iterate()
    dump("polarizability:h_atom:uhf", st)
    st.close(); s.close()
    # the O2 triplet followed to its minimum
    m = mol("oxygen/cc-pVDZ")
    s = q.System(m)
    s.set_schwarz(0.0)
    res = q.stabilize(s, q.HartreeFockConfig(2000, 1e-10), 9, 7)
    s.close()
    s, st = converged(m, True, 9, 7, density=res.density)
    dump("polarizability:oxygen/cc-pVDZ:uhf-minimum", st)
    st.close(); s.close()


def excitations():
    for name in ("h2@1.4/6-31G", "water/STO-3G", "water/6-31G", "water/cc-pVDZ", "ethylene/6-31G", "benzene/STO-3G"):
        s, st = converged(mol(name))
        dim = st.stability_dim(0)
        for method in ("cis", "tdhf"):
            for kind in (0, 1):          # (TDHF triplets of ethylene and benzene: the two refused references)
                r = st.excitations(method, kind=kind, nroots=min(8, dim), tol=1e-7, vectors=True)
                run = "excitations:%s:%s:k%d" % (name, method, kind)
                put(run, "energies", r.energies); put(run, "residuals", r.residuals); put(run, "vectors", r.vectors)
                put(run, "transition_dipole", r.transition_dipole); put(run, "oscillator", r.oscillator)
                put(run, "iterations", r.iterations); put(run, "products", r.products); put(run, "nconverged", r.nconverged)
                put(run, "converged", r.converged); put(run, "reference_unstable", r.reference_unstable)
        if name == "water/cc-pVDZ":
            for kind in (0, 1):
                P, M = st.excitation_matrices(kind)
                put("matrices:%s:k%d" % (name, kind), "ApB", P); put("matrices:%s:k%d" % (name, kind), "AmB", M)
        st.close(); s.close()


def mp2():
    for name, uhf, na, nb, frozen in (("water/cc-pVDZ", False, 0, 0, (0, 1)), ("oxygen/cc-pVDZ", True, 9, 7, (0,))):
        s, st = converged(mol(name), uhf, na, nb)
        for nf in frozen:
            o = st.mp2(nf)
            run = "mp2:%s:frozen%d" % (name, nf)
            put(run, "e_os", o.e_os); put(run, "e_ss", o.e_ss); put(run, "e_corr", o.e_corr)
        st.close(); s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["stability", "polarizability", "excitations", "mp2"])
    args = ap.parse_args()
    if not q.device_ready():
        raise SystemExit("subspace_ab: no gfx950 device")
    for name, f in (("stability", stability), ("polarizability", polarizability), ("excitations", excitations), ("mp2", mp2)):
        if args.only in (None, name):
            f()
            sys.stdout.flush()


if __name__ == "__main__":
    main()
