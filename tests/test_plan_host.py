"""Invariants of the work-list planner (qchem-rs_amd/csrc/qc_plan.cpp) on the CPU, read off the dump of the stand-alone program
tests/host/plan_dump_main.cpp.  The program is built here from that file, qc_system.cpp and qc_plan.cpp with the system C++ compiler and
-fsanitize=address,undefined (the HIP headers on the include path, the HIP runtime linked for an inline hipFree that never runs); nothing is
loaded into Python, a sanitizer report fails the run (exit status).  What is asserted holds for ANY planner - which quartet goes where and
how the lists are cut may change, these may not: every quartet is in exactly one class and, after screening, on exactly one rank; slots
and bundles cover each quartet's primitive quartets (and ket columns) exactly once; the sizes taken before the lists exist bound the later ones.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_system

PP_SWITCHED_OFF = ("QC_NO_BM_PP", "1")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    csrc = os.path.join(ROOT, "qchem-rs_amd", "csrc")
    exe = tmp_path_factory.mktemp("plan_dump") / "plan_dump_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(rocm, "include"), "-I", csrc, os.path.join(ROOT, "tests", "host", "plan_dump_main.cpp"),
                    os.path.join(csrc, "qc_system.cpp"), os.path.join(csrc, "qc_plan.cpp"), "-o", str(exe),
                    "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True, timeout=600)
    return str(exe)


_inputs, _dumps = {}, {}


def system_input(tmp_path_factory, mol, basis):
    """the arguments of qc_system_create in the program's input format, and the molecule"""
    if (mol, basis) not in _inputs:
        m = load_system(mol, basis)
        path = tmp_path_factory.mktemp("plan_in") / "system.bin"
        with open(path, "wb") as f:
            np.asarray([len(m.atoms), m.n_shells, len(m.exponents)], np.int32).tofile(f)
            for a in (m.atomic_numbers(), m.shell_atom, m.shell_L, m.shell_pure, m.shell_nprim):
                np.asarray(a, np.int32).tofile(f)
            for a in (m.coordinates(), m.exponents, m.coefficients):
                np.asarray(a, np.float64).tofile(f)
        _inputs[(mol, basis)] = (str(path), m)
    return _inputs[(mol, basis)]


class Dump:
    """the program's output, parsed (field order: the header of plan_dump_main.cpp)"""

    def __init__(self, text, mol):
        self.pairs, self.meta, self.classes = [], [], []
        for line in text.splitlines():
            w = line.split()
            tag, v = w[0], w[1:]
            if tag == "const":
                self.LREG, self.ITMAX, self.KET_BITS, self.LPAIR = map(int, v)
            elif tag == "sys":
                self.nbasis, self.nelec, self.npairs, self.rank, self.nranks, self.schwarz = map(int, v[:6])
                self.tau = float.fromhex(v[6])
            elif tag == "pair":
                f = list(map(int, v[1:14]))
                self.pairs.append(dict(K=f[1], na=f[2], nb=f[3], L=f[6], shA=f[10], shB=f[11], Kfull=f[12], Q=float.fromhex(v[17])))
            elif tag == "flags":
                self.pp_ok, self.has_fkets, self.merge_t1, self.merge_bm, self.nquartets, self.nscreened = map(int, v)
            elif tag == "meta":
                f = list(map(int, v[:12]))
                self.meta.append(dict(LAB=f[1], LCD=f[2], LGC=f[3], bm=f[4], slot_words=f[5], lds_bytes=f[6], col_slot_words=f[7], col_lds_bytes=f[8],
                                      col_lgc=f[9], bm_rows=f[10], ntasks=f[11]))
            elif tag == "class":
                f = list(map(int, v[:13])) + [float.fromhex(v[13]), float.fromhex(v[14])] + list(map(int, v[15:]))
                self.classes.append(dict(LAB=f[1], LCD=f[2], LGC=f[3], bm=f[4], slot_words=f[5], lds_bytes=f[6], col_slot_words=f[7], col_lds_bytes=f[8],
                                         col_lgc=f[9], bm_rows=f[10], ket_packed=f[11], prim_quartets=f[12], bytes_alg=f[13],
                                         flops_alg=f[14], lgc_widest=f[15], counts=tuple(f[16:21]), tasks=[], shard=[], slots=[], bundles=[], ketlist=[]))
            else:
                c = self.classes[int(v[0])]
                rec = tuple(map(int, v[1:]))
                {"t": c["tasks"], "s": c["shard"], "sl": c["slots"], "b": c["bundles"], "k": c["ketlist"]}[tag].append(rec if tag != "k" else rec[0])
        assert len(self.pairs) == self.npairs and len(self.meta) == len(self.classes)
        for c in self.classes:
            assert c["counts"] == tuple(len(c[k]) for k in ("tasks", "shard", "slots", "bundles", "ketlist"))
        self.shell_L = [int(x) for x in mol.shell_L]

    def is_pp(self, pair):
        return self.shell_L[self.pairs[pair]["shA"]] == 1 and self.shell_L[self.pairs[pair]["shB"]] == 1

    def ket_entry(self, c, entry):
        """(ket pair, first primitive, one past the last) of a ket-list entry - the decode qc_debug_ket_entry documents"""
        if not c["ket_packed"]:
            return entry, 0, self.pairs[entry]["K"]
        ket, kl0, n = entry & ((1 << self.KET_BITS) - 1), (entry >> self.KET_BITS) & 0x7F, (entry & 0xFFFFFFFF) >> (self.KET_BITS + 7)
        return (ket, 0, self.pairs[ket]["K"]) if n == 0 else (ket, kl0, kl0 + n)


@pytest.fixture(scope="module")
def dump(prog, tmp_path_factory):
    def run(mol, basis, switch=None, rank=0, nranks=1, schwarz=0):
        key = (mol, basis, switch, rank, nranks, schwarz)
        if key not in _dumps:
            path, m = system_input(tmp_path_factory, mol, basis)
            env = {k: v for k, v in os.environ.items() if not k.startswith("QC_")}
            if switch:
                env[switch[0]] = switch[1]
            p = subprocess.run([prog, path, str(rank), str(nranks), str(schwarz)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=120)
            assert p.returncode == 0, p.stderr[-4000:]
            _dumps[key] = Dump(p.stdout, m)
        return _dumps[key]
    return run


def exactly_once(rects, width, height):
    """the half-open rectangles (x0, x1, y0, y1) tile [0, width) x [0, height): inside it, not empty, pairwise disjoint, areas add up"""
    area = 0
    for i, (x0, x1, y0, y1) in enumerate(rects):
        if not (0 <= x0 < x1 <= width and 0 <= y0 < y1 <= height):
            return False
        area += (x1 - x0) * (y1 - y0)
        for a0, a1, b0, b1 in rects[:i]:
            if x0 < a1 and a0 < x1 and y0 < b1 and b0 < y1:
                return False
    return area == width * height


def check_classes(d, switch):
    """partition over classes; class membership"""
    seen = set()
    for c in d.classes:
        for bra, ket in c["tasks"]:
            key = (max(bra, ket), min(bra, ket))
            assert key not in seen
            seen.add(key)
            assert d.pairs[bra]["L"] == c["LAB"] and d.pairs[ket]["L"] == c["LCD"]
            if c["bm"] and (c["LAB"], c["LCD"]) == (2, 2):
                assert d.is_pp(ket)
        if c["bm"]:
            assert (c["LCD"] <= 1 and c["LAB"] + c["LCD"] <= d.LREG) or (c["LAB"], c["LCD"]) in ((4, 1), (2, 2))
        else:
            assert c["LGC"] in (c["lgc_widest"], 6)
    assert len(seen) == d.npairs * (d.npairs + 1) // 2
    has_pp_class = any(c["bm"] and (c["LAB"], c["LCD"]) == (2, 2) for c in d.classes)
    assert has_pp_class == (switch == ("QC_BM_PP_MIN", "1"))        # (water's list is short: only the override makes the class)


def check_column_class(d, c):
    by_task = {t: [] for t in c["shard"]}
    assert len(by_task) == len(c["shard"])
    lengths = []
    for bra, ket, lo, hi, c0, c1 in c["slots"]:
        ncd = d.pairs[ket]["na"] * d.pairs[ket]["nb"]
        assert hi - lo <= d.ITMAX
        assert (c0, c1) == (0, ncd) or (c0 % 16 == 0 and c1 == min(ncd, c0 + 16))
        by_task[(bra, ket)].append((lo, hi, c0, c1))                # (a slot of a quartet that is not in the shard: KeyError)
        lengths.append(hi - lo)
    for (bra, ket), rects in by_task.items():
        assert exactly_once(rects, d.pairs[bra]["K"] * d.pairs[ket]["K"], d.pairs[ket]["na"] * d.pairs[ket]["nb"]), (bra, ket)
    assert all(a >= b for a, b in zip(lengths, lengths[1:]))
    assert not c["bundles"] and not c["ketlist"]


def check_bra_major_class(d, c, switch):
    pp = (c["LAB"], c["LCD"]) == (2, 2)
    by_task = {(pad0, bra, ket): [] for bra, ket in c["shard"] for pad0 in ((0, 1, 2) if pp else (0,))}
    for bra, ij_lo, ij_hi, first, nket, maxK, pad0, pad1 in c["bundles"]:
        assert 1 <= nket <= 64 and 0 <= first and first + nket <= len(c["ketlist"])
        assert 0 <= ij_lo < ij_hi <= d.pairs[bra]["K"]
        longest = 0
        for e in c["ketlist"][first:first + nket]:
            ket, k0, k1 = d.ket_entry(c, e)
            longest = max(longest, k1 - k0)
            by_task[(pad0, bra, ket)].append((ij_lo, ij_hi, k0, k1))  # (one bra per bundle; a unit outside the shard or a wrong pad0: KeyError)
        assert maxK == longest
    for (pad0, bra, ket), rects in by_task.items():
        assert exactly_once(rects, d.pairs[bra]["K"], d.pairs[ket]["K"]), (pad0, bra, ket)
    if switch == ("QC_BM_UNIT", "0"):
        assert not c["ket_packed"]
    assert all(c["bm_rows"] >= d.pairs[bra]["na"] + d.pairs[bra]["nb"] for bra, _ in c["shard"])
    assert not c["slots"]


def check_lists(d, switch):
    for c, m in zip(d.classes, d.meta):
        assert set(c["shard"]) <= set(c["tasks"]) and len(set(c["shard"])) == len(c["shard"])
        if c["bm"]:
            check_bra_major_class(d, c, switch)
        else:
            check_column_class(d, c)
        assert (m["LAB"], m["LCD"], m["LGC"], m["bm"], m["ntasks"]) == (c["LAB"], c["LCD"], c["LGC"], c["bm"], len(c["tasks"]))
        for f in ("slot_words", "lds_bytes", "col_slot_words", "col_lds_bytes", "bm_rows"):
            assert m[f] >= c[f], f                                   # sizes before the lists exist: upper bounds for the allocation


CASES = [("water", "cc-pVDZ", None), ("water", "cc-pVDZ", ("QC_BM_PP_MIN", "1")), ("water", "cc-pVDZ", ("QC_BM_UNIT", "0")),
         ("water", "cc-pVDZ", PP_SWITCHED_OFF), ("water", "cc-pVTZ", None), ("water", "cc-pVTZ", ("QC_MFMA4_MAX", "0"))]


@pytest.mark.parametrize("mol,basis,switch", CASES, ids=lambda x: "=".join(x) if isinstance(x, tuple) else x)
def test_single_rank_lists_cover_every_quartet_once(dump, mol, basis, switch):
    d = dump(mol, basis, switch)
    check_classes(d, switch)
    for c in d.classes:
        assert sorted(c["shard"]) == sorted(c["tasks"])               # one rank, no Schwarz factors: the shard is the whole list
    assert d.nscreened == 0
    check_lists(d, switch)
    # what the case is there for
    packed = any(c["ket_packed"] for c in d.classes)
    assert packed == (switch != ("QC_BM_UNIT", "0"))
    split = any((c1 - c0) < d.pairs[ket]["na"] * d.pairs[ket]["nb"] for c in d.classes for _, ket, _, _, c0, c1 in c["slots"])
    lgc5_lcd4 = any(not c["bm"] and c["LAB"] >= 3 and c["LCD"] == 4 and c["LGC"] == 5 for c in d.classes)
    if basis == "cc-pVTZ":
        assert d.has_fkets and d.merge_t1 and split
        assert lgc5_lcd4 == (switch == ("QC_MFMA4_MAX", "0"))         # a short list: in the 64-lane instance unless switched off
    else:
        assert not d.has_fkets and not d.merge_t1 and not split


@pytest.mark.parametrize("mol,basis", [("water", "cc-pVDZ"), ("water", "cc-pVTZ")])
def test_three_ranks_with_schwarz_factors_deal_every_kept_quartet_once(dump, mol, basis):
    ds = [dump(mol, basis, None, r, 3, 1) for r in range(3)]
    d0 = ds[0]
    Q = [float("1e-%d" % (i % 15)) for i in range(d0.npairs)]         # the program's synthetic factors
    assert Q == [p["Q"] for p in d0.pairs]
    check_classes(d0, None)
    nkept = 0
    for ci, c in enumerate(d0.classes):
        kept = sorted(t for t in c["tasks"] if Q[t[0]] * Q[t[1]] >= d0.tau)
        dealt = sorted(t for d in ds for t in d.classes[ci]["shard"])
        assert dealt == kept
        assert all(sorted(d.classes[ci]["tasks"]) == sorted(c["tasks"]) for d in ds)
        nkept += len(kept)
    total = d0.npairs * (d0.npairs + 1) // 2
    assert 0 < nkept < total                                          # the screening branch did run, and did not drop everything
    for d in ds:
        assert d.nscreened == total - nkept
        check_lists(d, None)
