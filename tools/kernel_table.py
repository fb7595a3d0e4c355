"""The device code of two builds of the library, kernel by kernel: for every gfx950 code object in each shared library, every kernel symbol ->
(the instruction encodings of its body, its entry in the code object's metadata note).  Host-only (no GPU); the instrument for refactors that
move kernels between translation units or touch the host side only, the sibling of tools/plan_table.py.

    python tools/kernel_table.py <libA.so> <libB.so> [-v]

Prints the kernels that only one side has and the kernels whose encodings or metadata differ; exit status 1 if there are any.  The encodings are
the words llvm-objdump -d prints behind each instruction, WITHOUT the address column (a kernel that moved to another code object keeps its words,
not its address) and cut at the symbol's own size (the padding up to the next symbol belongs to the layout); the metadata is the kernel's item of
amdhsa.kernels in llvm-readelf --notes (registers, LDS, scratch, kernarg layout).  It compares; it does not look at what the instructions are."""
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _llvm(tool):
    from quick_amd.build import _hipcc
    for d in (os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(_hipcc()))), "llvm", "bin"), "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, tool)):
            return os.path.join(d, tool)
    found = shutil.which(tool)
    if not found:
        raise RuntimeError(tool + " not found next to hipcc, in /opt/rocm/llvm/bin or on PATH")
    return found


def _run(cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_objects(lib, tmp):
    """the gfx950 code objects of a shared library (one per translation unit with kernels), as ELF files under tmp"""
    fat = os.path.join(tmp, "fatbin")
    _run([_llvm("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "rest")])
    data = open(fat, "rb").read()
    out, at = [], data.find(_MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", data, at + len(_MAGIC))
        o = at + len(_MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, o)
            triple = data[o + 24:o + 24 + tl].decode()
            o += 24 + tl
            if "gfx950" in triple and size:
                out.append(os.path.join(tmp, "co%d.elf" % len(out)))
                with open(out[-1], "wb") as f:
                    f.write(data[at + off:at + off + size])
        at = data.find(_MAGIC, o)
    if not out:
        raise RuntimeError(lib + ": no gfx950 code object in .hip_fatbin (a compressed bundle?)")
    return out


_SYM = re.compile(r"^([0-9a-f]{16}) <(.+)>:$")
_INS = re.compile(r"// ([0-9A-F]+): ((?:[0-9A-F]{8} ?)+)\s*$")


def kernels_of(elf):
    """{kernel symbol: (encoding words, metadata text)} of one code object"""
    meta, name, item, inside = {}, None, [], False
    for line in _run([_llvm("llvm-readelf"), "--notes", elf]).splitlines() + ["end:"]:
        if line.startswith("amdhsa.kernels:"):
            inside = True
            continue
        if not inside:
            continue
        if line.startswith("  - ") or not line.startswith(" "):   # the next kernel's item, or the next top-level key
            if name:
                meta[name] = "\n".join(item)
            name, item = None, []
            if not line.startswith(" "):
                inside = False
                continue
        item.append(line)
        m = re.match(r"^\s+\.name:\s+(\S+)$", line.replace("  - ", "    ", 1))
        if m:
            name = m.group(1)
    size = {}
    for line in _run([_llvm("llvm-readelf"), "-s", "-W", elf]).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            size[f[7]] = (int(f[1], 16), int(f[2]))
    words, cur = {}, None
    for line in _run([_llvm("llvm-objdump"), "-d", elf]).splitlines():
        m = _SYM.match(line)
        if m:
            cur = m.group(2) if m.group(2) in meta else None
            if cur:
                words[cur] = []
            continue
        m = _INS.search(line) if cur else None
        if m and int(m.group(1), 16) < size[cur][0] + size[cur][1]:
            words[cur].extend(m.group(2).split())
    return {k: (" ".join(words.get(k, [])), meta[k]) for k in meta}


def table(lib):
    with tempfile.TemporaryDirectory() as tmp:
        out = {}
        for elf in code_objects(lib, tmp):
            for k, v in kernels_of(elf).items():
                if k in out and out[k] != v:
                    raise RuntimeError("%s: two code objects define %s differently" % (lib, k))
                out[k] = v
        return out


def main(argv):
    verbose = "-v" in argv
    libs = [a for a in argv if a != "-v"]
    if len(libs) != 2:
        print(__doc__)
        return 2
    a, b = table(libs[0]), table(libs[1])
    try:
        names = dict(zip(sorted(set(a) | set(b)), _run([_llvm("llvm-cxxfilt")] + sorted(set(a) | set(b))).splitlines()))
    except (RuntimeError, subprocess.CalledProcessError):
        names = {}
    show = lambda k: names.get(k, k)
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = [(k, a[k][0] != b[k][0], a[k][1] != b[k][1]) for k in sorted(set(a) & set(b)) if a[k] != b[k]]
    for k in only_a:
        print("only in %s: %s" % (libs[0], show(k)))
    for k in only_b:
        print("only in %s: %s" % (libs[1], show(k)))
    for k, enc, md in differ:
        print("differs (%s): %s" % (" + ".join(w for w, d in (("encoding", enc), ("metadata", md)) if d), show(k)))
        if verbose and md:
            print("  A: " + a[k][1].replace("\n", "\n     "))
            print("  B: " + b[k][1].replace("\n", "\n     "))
    print("%d kernels in %s, %d in %s: %d only in A, %d only in B, %d differ; %d instruction words compared"
          % (len(a), libs[0], len(b), libs[1], len(only_a), len(only_b), len(differ), sum(len(a[k][0].split()) for k in set(a) & set(b))))
    return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
