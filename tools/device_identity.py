#!/usr/bin/env python3
"""Is the kernel library's device code the same, symbol by symbol, as a git revision's?

  python tools/device_identity.py <rev> [extra hipcc flags, e.g. -DRM_BLOCK_TRACE]

Compiles the revision's csrc/ + include/ (unpacked as tools/build_variant.sh does) and the working
tree's with the flags of _build.py plus --cuda-device-only --no-gpu-bundle-output -c, and fails
unless
  * the sets of FUNC and OBJECT symbol names are equal (the per-compilation __hip_cuid_* aside),
  * every .text symbol's bytes are equal,
  * every .rodata symbol's bytes are equal, but for bytes 16-23 of a *.kd kernel descriptor
    (kernel_code_entry_byte_offset).
Whole-section hashes do not serve for a host-side change: kernels are emitted in the order the
host code instantiates them, so moving a launch moves every kernel after it (and its descriptor's
entry offset) while every function body stays byte for byte the same.
"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join("burn_raymarching_amd", "csrc", "rm_kernels.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-result",
         "--cuda-device-only", "--no-gpu-bundle-output", "-c"]


def tool(name):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if name == "hipcc":
        return hipcc
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (shutil.which(name), os.path.join(rocm, "llvm", "bin", name), os.path.join(rocm, "lib", "llvm", "bin", name)):
        if cand and os.path.exists(cand):
            return cand
    raise SystemExit(f"{name} not found")


def unpack(rev, dst):
    if rev == "WT":
        shutil.copytree(os.path.join(ROOT, "burn_raymarching_amd", "csrc"), os.path.join(dst, "burn_raymarching_amd", "csrc"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(dst, "include"))
    else:
        ar = subprocess.run(["git", "-C", ROOT, "archive", rev, "burn_raymarching_amd/csrc", "include"],
                            check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", dst], input=ar, check=True)


def symbols(obj):
    """{name: (section name, bytes)} of the FUNC and OBJECT symbols of a device code object."""
    readelf = tool("llvm-readelf")
    sections = {}  # index -> (name, file offset)
    for line in subprocess.run([readelf, "-S", "-W", obj], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines():
        line = line.strip()
        if not line.startswith("[") or line.startswith("[Nr]"):
            continue
        idx, rest = line[1:].split("]", 1)
        f = rest.split()
        if len(f) >= 5 and idx.strip().isdigit() and int(idx) > 0:
            sections[int(idx)] = (f[0], int(f[2], 16), int(f[3], 16))  # name type addr off size
    with open(obj, "rb") as fh:
        blob = fh.read()
    out = {}
    for line in subprocess.run([readelf, "-s", "-W", obj], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines():
        f = line.split()  # Num: Value Size Type Bind Vis Ndx Name
        if len(f) < 8 or f[3] not in ("FUNC", "OBJECT") or not f[6].isdigit() or f[7].startswith("__hip_cuid_"):
            continue
        sec, addr, off = sections[int(f[6])]
        size = int(f[2], 0)
        start = off + int(f[1], 16) - addr  # the device object is linked: values are addresses
        out[f[7]] = (sec, blob[start:start + size] if sec != ".bss" else b"\0" * size)
    return out


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    rev, extra = sys.argv[1], sys.argv[2:]
    syms = {}
    with tempfile.TemporaryDirectory() as tmp:
        procs = {}
        for name, what in (("rev", rev), ("tree", "WT")):
            d = os.path.join(tmp, name)
            os.makedirs(d)
            unpack(what, d)
            procs[name] = subprocess.Popen([tool("hipcc")] + FLAGS + extra + ["-o", "dev.o", SRC], cwd=d)
        for name, p in procs.items():
            if p.wait() != 0:
                raise SystemExit(f"compiling {name} failed")
            syms[name] = symbols(os.path.join(tmp, name, "dev.o"))
    a, b = syms["rev"], syms["tree"]
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", rev], stdout=subprocess.PIPE, text=True).stdout.strip()
    print(f"# device code of the working tree against {rev} ({sha}); flags: {' '.join(FLAGS + extra)}")
    bad = [f"only in {rev}: {n}" for n in sorted(set(a) - set(b))] + [f"only in the tree: {n}" for n in sorted(set(b) - set(a))]
    count = {}
    for n in sorted(set(a) & set(b)):
        (sa, xa), (sb, xb) = a[n], b[n]
        if n.endswith(".kd") and len(xa) == 64 and len(xb) == 64:  # entry offset: where the kernel landed
            xa, xb = xa[:16] + xa[24:], xb[:16] + xb[24:]
        if sa != sb or xa != xb:
            bad.append(f"differs: {n} ({sa} {len(xa)} B / {sb} {len(xb)} B)")
        count[sa] = count.get(sa, (0, 0))
        count[sa] = (count[sa][0] + 1, count[sa][1] + len(xa))
    for sec, (k, nbytes) in sorted(count.items()):
        print(f"{sec}: {k} symbols, {nbytes} bytes compared")
    print(f"symbols: {len(a)} in {rev}, {len(b)} in the tree")
    for line in bad:
        print(line)
    print("IDENTICAL" if not bad else f"NOT IDENTICAL ({len(bad)} findings)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
