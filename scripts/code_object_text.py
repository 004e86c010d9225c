"""Device code of the built objects: per .o of a library directory its name, the sha256 of the .text section of its gfx950 code
object and the number of kernels.  Two builds with equal tables run the same device code (whole code objects differ between builds
of equivalent sources: they carry a hash of the source text).
    python scripts/code_object_text.py [directory]      (default: hypad_amd/lib; the development library's objects: hypad_amd/lib/dev)
    python scripts/code_object_text.py --kernels [directory]
        per kernel (every symbol with a kernel descriptor, `<name>.kd`) one line `sha256-of-its-own-bytes  object  mangled-name`: the
        bytes [address, address + size) of the symbol table's entry.  For builds between which kernels changed objects: the lines
        without their object column, sorted, are equal when every kernel's code is."""
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hypad_amd import build  # noqa: E402


def kernel_digests(co, text):
    """{mangled kernel name: sha256 of its bytes} of the code object `co`, whose .text section was dumped into the file `text`"""
    readelf = os.path.join(build.LLVM_BIN, "llvm-readelf")
    base = None
    for line in subprocess.run([readelf, "-S", "--wide", co], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) > 3 and f[1] == ".text":
            base = int(f[3], 16)
    code = open(text, "rb").read()
    funcs, descriptors = {}, set()
    for line in subprocess.run([readelf, "-s", "--wide", co], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.split()                                   # Num: Value Size Type Bind Vis Ndx Name
        if len(f) != 8 or not f[0].endswith(":"):
            continue
        if f[3] == "FUNC":
            funcs[f[7]] = (int(f[1], 16), int(f[2]))
        elif f[7].endswith(".kd"):
            descriptors.add(f[7][:-3])
    out = {}
    for name in sorted(descriptors):
        addr, size = funcs[name]
        assert base is not None and base <= addr and addr - base + size <= len(code), name
        out[name] = hashlib.sha256(code[addr - base:addr - base + size]).hexdigest()
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--kernels"]
    per_kernel = "--kernels" in sys.argv[1:]
    objdir = args[0] if args else build.LIB_DIR
    for f in sorted(os.listdir(objdir)):
        if not f.endswith(".o"):
            continue
        with tempfile.TemporaryDirectory() as d:
            co, text = os.path.join(d, "gfx950.co"), os.path.join(d, "text.bin")
            if not build.gfx950_code_object(os.path.join(objdir, f), co):
                continue                                   # (host-only object)
            subprocess.check_call([os.path.join(build.LLVM_BIN, "llvm-objcopy"), "--dump-section=.text=" + text, co])
            digest = hashlib.sha256(open(text, "rb").read()).hexdigest()
            kernels = kernel_digests(co, text) if per_kernel else {}
        if per_kernel:
            for name, h in kernels.items():
                print("%s  %-16s %s" % (h, f, name))
        else:
            print("%-16s %s %4d kernels" % (f, digest, len(build.kernel_metadata(os.path.join(objdir, f)))))
