#!/usr/bin/env python3
"""SHA-256 of every kernel's device code in csrc/*.hip units, cross-compiled for gfx950 with the product's flags: the
listing two trees are compared by when a change must not move an instruction (no GPU, no torch -- the counterpart, for
device code, of tools/tri_digests.py for outputs; docs/EXPERIMENTS.md, part K).

A kernel's body runs from its label to the end of its `.amdhsa_kernel` descriptor block.  Blank lines and lines that are
only a comment (`;`-only, `;;#ASMSTART` / `;;#ASMEND` among them) are dropped, and so is a line's trailing comment; instructions, labels, directives and the
descriptor all count; the kernel's own symbol is hashed as a placeholder and its local labels without the kernel's
ordinal in the unit (a re-parameterised kernel, or one whose neighbours moved to another unit, keeps its digest).
One line per kernel: name, instruction count, digest.

    python tools/kernel_digests.py sphere_raster data_to_model > listing.txt      (in each tree; then `diff`)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spherehand_amd import build  # noqa: E402


def assembly(unit):
    out = os.path.join(tempfile.mkdtemp(), unit + ".s")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.check_call([build.HIPCC] + flags + ["-S", "--cuda-device-only", "-I", os.path.join(ROOT, "include"), "-I",
                                                   os.path.join(build.PKG, "csrc"), "-o", out,
                                                   os.path.join(build.PKG, "csrc", unit + ".hip")], stderr=subprocess.DEVNULL)
    return open(out).read().split("\n")


def kernels(lines):
    """(mangled name, normalised body lines) of every kernel, in the file's order."""
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l)]
    for n, i in enumerate(starts):
        body = lines[i:starts[n + 1] if n + 1 < len(starts) else len(lines)]
        ends = [k for k, l in enumerate(body) if l.strip() == ".end_amdhsa_kernel"]
        if not ends:                 # a device function that was not inlined: no descriptor, not a kernel
            continue
        kept = [l.split(" ; @")[0] if k == 0 else l for k, l in enumerate(body[:ends[0] + 1])
                if l.strip() and not l.strip().startswith(";")]
        name = lines[i].split(":")[0]
        # the kernel's own symbol (its encoding after `_Z`: labels, descriptor, the names of its static LDS) by a fixed
        # placeholder, its ordinal in the unit out of its local labels (.LBB<ordinal>_<n>, .Lfunc_end<ordinal>) and no
        # trailing notes (they name labels too), so that a kernel whose template parameters or whose neighbours in the
        # unit change -- and nothing else -- keeps its digest
        yield name, [re.sub(r"\.(LBB|Lfunc_end)\d+", r".\1", l.split(";")[0].rstrip().replace(name[2:], "KERNEL")) for l in kept]


for unit in sys.argv[1:] or ["sphere_raster"]:
    names, listing = [], []
    for name, body in kernels(assembly(unit)):
        code = body[:next(k for k, l in enumerate(body) if l.strip().startswith(".section"))]
        count = sum(1 for l in code if re.match(r"^\s+[a-z]", l))
        names.append(name)
        listing.append((count, hashlib.sha256("\n".join(body).encode()).hexdigest()))
    short = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    for name, full, (count, digest) in zip(names, short, listing):
        print("%s %s %6d %s" % (unit, re.sub(r"^void ", "", full or name).split("(")[0].replace(" ", ""), count, digest))
