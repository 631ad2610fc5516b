"""Instruction mix of named kernels, from gfx950 assembly or code objects (no GPU needed):
    python tools/isa_mix.py KERNEL_SUBSTRING name=file [name=file ...]
`file` is a .s file (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S x.hip), a code object, or a library whose .hip_fatbin
bundles are searched (tools/kernel_resources.py).  For every kernel whose demangled name contains the substring it prints one markdown
column: code bytes, VGPR, AGPR and SGPR counts, both spill counts, scratch bytes, the number of instructions, and a histogram by class, then
two single counts: global accesses that carry a 64-bit vector address (`v[lo:hi], off`, not the scalar-base form) and `v_lshl_add_u64`.
The classes are static counts of the kernel's own symbol; functions it calls are listed below the table with their sizes."""
import os, re, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import code_objects  # noqa: E402

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size")
CLASSES = ("MFMA", "f64 VALU arithmetic", "other VALU", "lane moves", "accumulator moves", "LDS", "global", "scalar memory", "SALU",
           "exec-mask operations", "branches", "waits", "barriers", "nops")
F64_ARITH = re.compile(r"v_(fma|fmac|mul|add|div_scale|div_fmas|div_fixup|rcp|rsq|sqrt|max|min|ldexp|frexp_mant|trunc|floor|ceil|rndne|fract)_f64")


def classify(op, operands):
    if op.startswith("v_mfma") or op.startswith("v_smfmac"): return "MFMA"
    if op.startswith("v_accvgpr"): return "accumulator moves"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane", "v_permlane", "ds_bpermute", "ds_permute", "ds_swizzle")) or "dpp" in op or "row_" in operands or "quad_perm" in operands:
        return "lane moves"
    if op.startswith("ds_"): return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")): return "global"
    if op.startswith("v_"): return "f64 VALU arithmetic" if F64_ARITH.match(op) else "other VALU"
    if op.startswith(("s_load", "s_buffer_load")): return "scalar memory"
    if op.startswith("s_waitcnt"): return "waits"
    if op == "s_barrier": return "barriers"
    if op in ("s_nop", "s_sleep"): return "nops"
    if op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_call", "s_endpgm")): return "branches"
    if "saveexec" in op or re.search(r"\bexec(_lo|_hi)?\b", operands): return "exec-mask operations"
    if op.startswith("s_"): return "SALU"
    return "other VALU"


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True)
    return dict(zip(names, (re.sub(r"^void ", "", l) for l in p.stdout.splitlines())))


def metadata(notes):
    """{kernel symbol: {field: int}} from the amdhsa.kernels note (as text of llvm-readelf --notes or of a .s file)."""
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
        block = "  - .agpr_count:" + block
        block = block.split("amdhsa.target")[0]
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(m.group(1)) if (m := re.search(re.escape(k) + r":\s+(\d+)", block)) else 0 for k in META}
    return out


def functions_of_asm(text):
    """{symbol: (code bytes, [(opcode, operands)])} of a .s file."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^([A-Za-z_][\w.$]*):", line)
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1); out[cur] = [0, []]; continue
        if cur is None: continue
        if re.match(r"^\.Lfunc_end", line): cur = None; continue
        m = re.search(r"; codeLenInByte = (\d+)", line)
        if m: out[cur][0] = int(m.group(1)); continue
        m = re.match(r"^\s+([a-z]\w+)\s*([^;]*)", line)
        if m and not line.lstrip().startswith("."): out[cur][1].append((m.group(1), m.group(2)))
    # (codeLenInByte stands in the comment block behind .Lfunc_end)
    for m in re.finditer(r"\n; Kernel info:\n; codeLenInByte = (\d+)", text):
        name = re.findall(r"\n\t\.size\t(\S+), \.Lfunc_end", text[:m.start()])
        if name and name[-1] in out: out[name[-1]][0] = int(m.group(1))
    return {k: (v[0], v[1]) for k, v in out.items() if v[1]}


def functions_of_object(path):
    """{symbol: (code bytes, [(opcode, operands)])} of a code object."""
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    size = {r[7]: int(r[2]) for r in (l.split() for l in syms.splitlines()) if len(r) == 8 and r[3] == "FUNC"}
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m: cur = m.group(1); out[cur] = []; continue
        m = re.match(r"^\s+([a-z]\w+)\s*([^/]*)", line)
        if m and cur: out[cur].append((m.group(1), m.group(2)))
    return {k: (size.get(k, 0), v) for k, v in out.items() if v}


def load(path):
    """[(functions, metadata)] of the file's code objects."""
    if path.endswith(".s"):
        text = open(path).read()
        return [(functions_of_asm(text), metadata(text))]
    blob = open(path, "rb").read()
    objs = [blob] if blob[:4] == b"\x7fELF" and b"__CLANG_OFFLOAD_BUNDLE__" not in blob else code_objects(path)
    out = []
    for o in objs:
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(o); f.flush()
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], stdout=subprocess.PIPE, text=True, check=True).stdout
            out.append((functions_of_object(f.name), metadata(notes)))
    return out


if __name__ == "__main__":
    want, files = sys.argv[1], [a.split("=", 1) for a in sys.argv[2:]]
    cols, callees = [], []
    for label, path in files:
        for funcs, meta in load(path):
            short = demangle(list(funcs))
            if not any(want in short[k] and k in meta for k in funcs): continue
            for k in sorted(funcs):
                if k in meta and want in short[k]:
                    nbytes, ins = funcs[k]
                    hist = dict.fromkeys(CLASSES, 0)
                    for op, operands in ins: hist[classify(op, operands)] += 1
                    top = {}
                    for op, _ in ins: top[op] = top.get(op, 0) + 1
                    hist["global, 64-bit vector address"] = sum(1 for op, operands in ins if classify(op, operands) == "global" and operands.rstrip().endswith(", off"))
                    hist["v_lshl_add_u64"] = top.get("v_lshl_add_u64", 0)
                    cols.append((label, re.sub(r"\(.*$", "", short[k]), nbytes, meta[k], len(ins), hist, sorted(top.items(), key=lambda x: -x[1])[:6]))
                elif k not in meta:
                    callees.append((label, short[k], funcs[k][0], len(funcs[k][1])))
    rows = [("code bytes", lambda c: c[2]), ("VGPR", lambda c: c[3][".vgpr_count"] - c[3][".agpr_count"]), ("AGPR", lambda c: c[3][".agpr_count"]),
            ("SGPR", lambda c: c[3][".sgpr_count"]), ("SGPR spills", lambda c: c[3][".sgpr_spill_count"]),
            ("VGPR spills", lambda c: c[3][".vgpr_spill_count"]), ("scratch bytes", lambda c: c[3][".private_segment_fixed_size"]),
            ("instructions", lambda c: c[4])] + [(cl, (lambda c, cl=cl: c[5][cl])) for cl in CLASSES + ("global, 64-bit vector address", "v_lshl_add_u64")] + \
           [("most frequent", lambda c: ", ".join("%s %d" % t for t in c[6]))]
    print("| | " + " | ".join("%s: `%s`" % (c[0], c[1]) for c in cols) + " |\n|---|" + "---|" * len(cols))
    for name, f in rows:
        print("| %s | %s |" % (name, " | ".join(str(f(c)) for c in cols)))
    if callees:
        print("\nFunctions beside the kernels in the same code objects (not in the counts above):\n")
        for label, name, nbytes, n in callees: print("* %s: `%s`, %d bytes, %d instructions" % (label, name, nbytes, n))
