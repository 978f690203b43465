#!/usr/bin/env python3
"""Per-kernel register / scratch / code-size table of a built libtrajopt_grpo_hip.so, read from its gfx950 code objects (no GPU).

    tools/kernel_resources.py LIB.so [--match REGEX]            # one TSV line per kernel
    tools/kernel_resources.py NEW.so --against OLD.so [--match REGEX] [--size-may-differ REGEX]
        # every kernel of OLD must exist in NEW under the same mangled name with the same .vgpr_count, .sgpr_count,
        # .private_segment_fixed_size and code size; exit status 1 and one line per difference otherwise
        # --size-may-differ: kernels whose name matches may differ in code size alone (one SIZE line each, not a failure)

The library's .hip_fatbin section is a run of clang offload bundles (one per translation unit); each holds one ELF code object
whose AMDGPU metadata note lists the kernels.  Needs llvm-objcopy / llvm-readelf (ROCM_LLVM_BIN, default /opt/rocm/llvm/bin).
"""
import argparse
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib, tmp):
    fat = os.path.join(tmp, "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(tmp, "copy.so")])
    blob = open(fat, "rb").read()
    out, pos = [], blob.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", blob, pos + len(MAGIC))
        q = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tlen].decode()
            q += 24 + tlen
            if "amdgcn" in triple and size:
                path = os.path.join(tmp, f"co{len(out)}.elf")
                open(path, "wb").write(blob[pos + off:pos + off + size])
                out.append(path)
        pos = blob.find(MAGIC, q)
    return out


def kernels(lib):
    """mangled kernel name -> dict(vgpr, agpr, sgpr, scratch, lds, size)"""
    table = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
            syms = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-sW", co], text=True)
            sizes = {}
            for line in syms.splitlines():
                f = line.split()
                if len(f) >= 8 and f[3] == "FUNC":
                    sizes[f[7]] = int(f[2], 0)
            for block in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
                block = ".agpr_count:" + block

                def field(name, default=None):
                    m = re.search(r"\." + name + r":\s*'?([^'\n]+)'?", block)
                    return m.group(1).strip() if m else default
                name = field("name")
                if name is None:
                    continue
                table[name] = dict(vgpr=int(field("vgpr_count", 0)), agpr=int(field("agpr_count", 0)), sgpr=int(field("sgpr_count", 0)),
                                   scratch=int(field("private_segment_fixed_size", 0)), lds=int(field("group_segment_fixed_size", 0)),
                                   size=sizes.get(name, -1))
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lib")
    ap.add_argument("--against")
    ap.add_argument("--match", default=".")
    ap.add_argument("--size-may-differ", default=None, metavar="REGEX")
    a = ap.parse_args()
    new = kernels(a.lib)
    pat = re.compile(a.match)
    if a.against is None:
        print("kernel\tvgpr\tagpr\tsgpr\tscratch\tcode_bytes")
        for name in sorted(new):
            if pat.search(name):
                k = new[name]
                print(f"{name}\t{k['vgpr']}\t{k['agpr']}\t{k['sgpr']}\t{k['scratch']}\t{k['size']}")
        return 0
    old = kernels(a.against)
    bad = 0
    checked = 0
    resized = 0
    size_pat = re.compile(a.size_may_differ) if a.size_may_differ else None
    for name in sorted(old):
        if not pat.search(name):
            continue
        checked += 1
        if name not in new:
            print(f"MISSING\t{name}")
            bad += 1
        elif size_pat is not None and size_pat.search(name) and dict(new[name], size=0) == dict(old[name], size=0):
            if new[name]["size"] != old[name]["size"]:
                print(f"SIZE\t{name}\t{old[name]['size']} -> {new[name]['size']} ({new[name]['size'] - old[name]['size']:+d})\t{old[name]}")
                resized += 1
        elif new[name] != old[name]:
            print(f"DIFFERS\t{name}\told {old[name]}\tnew {new[name]}")
            bad += 1
    print(f"{checked} kernels of {a.against} checked against {a.lib}: {bad} differ"
          + (f", {resized} differ in code size alone" if size_pat is not None else "") + f"; {len(set(new) - set(old))} kernels are new")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
