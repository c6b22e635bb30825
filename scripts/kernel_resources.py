#!/usr/bin/env python3
"""Registers, scratch, LDS and a listing hash of every kernel of the library, one line per kernel.

    python scripts/kernel_resources.py [--keep DIR] > profiles/kernel_resources_after.txt

Needs no GPU.  Every .hip of build.py's SOURCES is compiled for the device only, with build.py's FLAGS and EXTRA_FLAGS, to
assembly.  Per kernel: ``source name vgpr agpr sgpr scratch lds lines sha256`` -- the counts and the private- and group-segment
sizes (bytes) come from the kernel metadata at the end of the assembly file; ``lines`` is the number of instruction lines between
the kernel's label and its end label, and the hash is taken over those lines and the labels between them, comments and
directives stripped (block labels lose the function's number, which depends on the kernel's position in its file).  Two
commits that print the same line for a kernel launch the same machine code for it, up to the functions it calls.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ultranest_amd", "csrc")
sys.path.insert(0, CSRC)

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def assemble(build, src, directory):
    out = os.path.join(directory, src.replace(".hip", ".s"))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + build.FLAGS + build.EXTRA_FLAGS.get(src, []) + ["--cuda-device-only", "-S", os.path.join(CSRC, src), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    with open(out) as fh:
        return fh.read().splitlines()


def metadata(lines):
    """{kernel name: {field: value}} from the amdhsa.kernels list"""
    first = lines.index("amdhsa.kernels:")
    kernels = []
    for line in lines[first + 1:]:
        if not line.startswith(" "):
            break
        m = re.match(r"^  (- | {2})(\.\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            kernels.append({})
        kernels[-1][m.group(2)] = m.group(3).strip().strip("'")
    return {k[".name"]: k for k in kernels}


def listing(texts, name):
    """instruction lines and labels of one function: from its label to its end label (texts: the lines without comments)"""
    out = []
    for text in texts[texts.index(name + ":") + 1:]:
        if text.startswith(".Lfunc_end"):
            break
        if not text or (text.startswith(".") and not text.endswith(":")):
            continue
        out.append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return out


def main():
    import build
    with tempfile.TemporaryDirectory() as tmp:
        if len(sys.argv) > 2 and sys.argv[1] == "--keep":      # leave the assembly files in this directory
            tmp = sys.argv[2]
            os.makedirs(tmp, exist_ok=True)
        with ThreadPoolExecutor(max_workers=8) as ex:
            files = list(ex.map(lambda s: assemble(build, s, tmp), build.SOURCES))
    for src, lines in zip(build.SOURCES, files):
        if "amdhsa.kernels:" not in lines:
            continue
        meta = metadata(lines)
        texts = [line.split(";")[0].strip() for line in lines]
        for name in sorted(meta):
            body = listing(texts, name)
            ninstr = sum(1 for t in body if not t.endswith(":"))
            digest = hashlib.sha256("\n".join(body).encode()).hexdigest()[:16]
            print(src, name, *[meta[name].get(f, "0") for f in FIELDS], ninstr, digest)


if __name__ == "__main__":
    main()
