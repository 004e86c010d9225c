"""Device code of the built objects: per .o of a library directory its name, the sha256 of the .text section of its gfx950 code
object and the number of kernels.  Two builds with equal tables run the same device code (whole code objects differ between builds
of equivalent sources: they carry a hash of the source text).
    python scripts/code_object_text.py [directory]      (default: hypad_amd/lib; the development library's objects: hypad_amd/lib/dev)"""
import hashlib
import os
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hypad_amd import build  # noqa: E402

if __name__ == "__main__":
    objdir = sys.argv[1] if len(sys.argv) > 1 else build.LIB_DIR
    for f in sorted(os.listdir(objdir)):
        if not f.endswith(".o"):
            continue
        with tempfile.TemporaryDirectory() as d:
            co, text = os.path.join(d, "gfx950.co"), os.path.join(d, "text.bin")
            if not build.gfx950_code_object(os.path.join(objdir, f), co):
                continue                                   # (host-only object)
            subprocess.check_call([os.path.join(build.LLVM_BIN, "llvm-objcopy"), "--dump-section=.text=" + text, co])
            digest = hashlib.sha256(open(text, "rb").read()).hexdigest()
        print("%-16s %s %4d kernels" % (f, digest, len(build.kernel_metadata(os.path.join(objdir, f)))))
