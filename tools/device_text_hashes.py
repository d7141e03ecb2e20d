#!/usr/bin/env python
"""SHA-256 of the .text section of every gfx950 code object of a library: two builds whose hashes agree contain byte-identical
kernels (what a refactoring of the kernel sources must show).    python tools/device_text_hashes.py [--per-kernel] [lib.so | object.o]

--per-kernel   one line per function symbol of every code object -- symbol, size, SHA-256 of its bytes -- sorted by symbol: a change of
               the order in which a translation unit instantiates its kernels moves the whole-section hash although no kernel changed,
               and `diff` of two such listings names the kernels that did.  Hashes of bytes only; no instruction is inspected."""
import sys as _sys
if {"-h", "--help"} & set(_sys.argv[1:]):          # every tool answers --help without touching the GPU
    print(__doc__)
    raise SystemExit(0)
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_hazards as ih  # noqa: E402


def _text(obj):
    text = obj + ".text"
    subprocess.run([os.path.join(ih.LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.text", obj, text], check=True)
    return open(text, "rb").read()


def hashes(lib):
    out = []
    with tempfile.TemporaryDirectory() as wd:
        for obj in ih.code_objects(lib, wd):
            text = _text(obj)
            out.append((os.path.basename(obj).split(".hipv4")[0].split(".")[-1], len(text), hashlib.sha256(text).hexdigest()))
    return out


def kernel_hashes(lib):
    """[(symbol, size, sha256)] over the function symbols of every code object of `lib`, sorted by symbol."""
    readelf = os.path.join(ih.LLVM, "llvm-readelf")
    out = []
    with tempfile.TemporaryDirectory() as wd:
        for obj in ih.code_objects(lib, wd):
            text = _text(obj)
            base = None
            for ln in subprocess.run([readelf, "-S", "-W", obj], check=True, capture_output=True, text=True).stdout.split("\n"):
                f = ln.replace("[", " ").replace("]", " ").split()
                if len(f) > 3 and f[1] == ".text":
                    base = int(f[3], 16)
            for ln in subprocess.run([readelf, "-s", "-W", obj], check=True, capture_output=True, text=True).stdout.split("\n"):
                f = ln.split()            # Num: Value Size Type Bind Vis Ndx Name
                if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND" and int(f[2]) > 0:
                    lo = int(f[1], 16) - base
                    body = text[lo:lo + int(f[2])]
                    assert len(body) == int(f[2]), f[7]
                    out.append((f[7], len(body), hashlib.sha256(body).hexdigest()))
    return sorted(set(out))       # (a linked code object lists its kernels in .dynsym and in .symtab)


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x != "--per-kernel"]
    lib = args[0] if args else ih.DEFAULT_LIB
    if "--per-kernel" in sys.argv[1:]:
        for sym, size, h in kernel_hashes(lib):
            print("%s %d %s" % (sym, size, h))
    else:
        for idx, size, h in hashes(lib):
            print("code object %s: .text %d bytes  sha256 %s" % (idx, size, h))
