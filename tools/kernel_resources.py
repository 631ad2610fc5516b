"""Kernel resources of library builds side by side, from their gfx950 code objects (no GPU needed):
    python tools/kernel_resources.py [--filter SUBSTRING] name=lib.so [name=lib.so ...]
Every bundle of a library's .hip_fatbin section (one per translation unit with device code) is cut out, hashed and its kernels' metadata
read with llvm-readelf: VGPR, AGPR, SGPR, scratch bytes, static LDS bytes, and the waves per SIMD that the registers allow (512 per lane
and SIMD, allocated in blocks of 8; dynamic LDS is not in the metadata).  Prints two markdown tables: the code objects with their
hashes (equal across all the libraries or not), then one row per kernel with one column group per library."""
import hashlib, os, re, struct, subprocess, sys, tempfile

READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def code_objects(lib):
    """The gfx950 code objects of `lib`, in file order."""
    blob, out = open(lib, "rb").read(), []
    for m in re.finditer(re.escape(MAGIC), blob):
        p = m.start() + len(MAGIC)
        (n,) = struct.unpack_from("<Q", blob, p); p += 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p); p += 24
            triple = blob[p:p + tl].decode(); p += tl
            if "gfx950" in triple:
                out.append(blob[m.start() + off:m.start() + off + size])
    return out


def kernels(obj):
    """{kernel name: (vgpr, agpr, sgpr, scratch, static lds)} of one code object."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(obj); f.flush()
        notes = subprocess.run([READELF, "--notes", f.name], stdout=subprocess.PIPE, text=True, check=True).stdout
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
        block = "  - .agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block)
        vals = [re.search(re.escape(k) + r":\s+(\d+)", block) for k in FIELDS]
        if name and all(vals):
            out[name.group(1)] = tuple(int(v.group(1)) for v in vals)
    return out


def demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True)
    # (kernels in an unnamed namespace demangle to "(anonymous namespace)::name<..>(args)": that prefix goes, then the argument list)
    return dict(zip(names, (re.sub(r"^void |\(.*$", "", l.replace("(anonymous namespace)::", "")) for l in p.stdout.splitlines())))


def waves(vgpr, agpr):
    return min(8, 512 // max(8, (vgpr + agpr + 7) // 8 * 8))     # (vgpr, agpr: the two parts of the unified file)


if __name__ == "__main__":
    args = sys.argv[1:]
    flt = args.pop(args.index("--filter") + 1) if "--filter" in args else ""
    libs = [a.split("=", 1) for a in args if a != "--filter"]
    objs = {n: code_objects(p) for n, p in libs}
    names = [n for n, _ in libs]
    count = max(len(o) for o in objs.values())
    print("| code object | kernels | " + " | ".join("%s: bytes, sha256 (first 32 digits)" % n for n in names) + " | equal |\n|---|---|" + "---|" * (len(names) + 1))
    res = {n: {} for n in names}
    for i in range(count):
        row, hashes, nk = [], set(), 0
        for n in names:
            o = objs[n][i] if i < len(objs[n]) else b""
            h = hashlib.sha256(o).hexdigest()[:32]; hashes.add(h)
            k = kernels(o) if o else {}
            nk = len(k)
            for name, v in k.items(): res[n][name] = v + (i,)
            row.append("%d `%s`" % (len(o), h))
        print("| %d | %d | %s | %s |" % (i, nk, " | ".join(row), "yes" if len(hashes) == 1 else "no"))
    allk = sorted({k for n in names for k in res[n]})
    short = demangle(allk)
    print("\n| kernel (code object) | " + " | ".join("%s: VGPR + AGPR, SGPR, scratch B, static LDS B, waves/SIMD" % n for n in names) + " |\n|---|" + "---|" * len(names))
    for k in allk:
        if flt not in short[k]: continue
        cells = []
        for n in names:
            v = res[n].get(k)
            cells.append("%d + %d, %d, %d, %d, %d" % (v[0] - v[1], v[1], v[2], v[3], v[4], waves(v[0] - v[1], v[1])) if v else "-")   # (.vgpr_count is the total)
        co = next(res[n][k][5] for n in names if k in res[n])
        print("| `%s` (%d) | %s |" % (short[k], co, " | ".join(cells)))
