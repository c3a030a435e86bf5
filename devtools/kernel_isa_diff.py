#!/usr/bin/env python3
"""Compare the gfx950 kernels of two libfedrann_hip.so builds (no GPU needed).

    python devtools/kernel_isa_diff.py OLD.so NEW.so [--arch gfx950] [--show N]

For every kernel symbol: is the metadata equal (VGPR / AGPR / SGPR counts, private segment = scratch, group segment =
LDS, kernarg size and argument layout), and is the disassembly equal?  Disassembly is compared per kernel, so the
order of the functions in the code object does not matter, and modulo pc-relative displacements to other symbols
(the literals added to an s_getpc_b64 result).  Branches inside a kernel are relative to the kernel's own code and
are compared as they are.  Exit status 1 if anything differs or a kernel exists on one side only.

Uses llvm-objcopy, clang-offload-bundler, llvm-readelf and llvm-objdump from the ROCm LLVM directory
(ROCM_PATH, default /opt/rocm).
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

META_FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size",
               "kernarg_segment_size", "wavefront_size", "max_flat_workgroup_size")


def llvm_tool(name):
    root = os.environ.get("ROCM_PATH", "/opt/rocm")
    for d in (os.path.join(root, "llvm", "bin"), os.path.join(root, "lib", "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    raise SystemExit(f"{name} not found under {root}")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(lib, arch, tmp, tag):
    fatbin, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    # (an output file of its own: without one llvm-objcopy rewrites the library in place)
    run(llvm_tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fatbin, lib, os.path.join(tmp, tag + ".copy"))
    run(llvm_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fatbin, "--output=" + co,
        "--targets=hipv4-amdgcn-amd-amdhsa--" + arch)
    if not os.path.getsize(co):
        raise SystemExit(f"{lib}: no {arch} code object")
    return co


def metadata(co):
    """{kernel symbol: {field: value, 'args': [(offset, size, kind), ...]}} from the amdhsa.kernels note."""
    kernels, cur, arg = [], None, None
    for line in run(llvm_tool("llvm-readelf"), "--notes", co).splitlines():
        m = re.match(r"^(\s*)(- )?\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        indent, dash, key, val = len(m.group(1)), bool(m.group(2)), m.group(3), m.group(4).strip("'\" ")
        if indent <= 2 and dash:  # a new entry of amdhsa.kernels (its fields: indent 4; its .args entries: deeper)
            cur, arg = {"args": []}, None
            kernels.append(cur)
        if cur is None:
            continue
        if indent > 4:  # inside .args
            if dash:
                arg = {}
                cur["args"].append(arg)
            if arg is not None and key in ("offset", "size", "value_kind"):
                arg[key] = val
        elif key in META_FIELDS or key == "name":
            cur[key] = val
    out = {}
    for k in kernels:
        if "name" in k:
            k["args"] = [(a.get("offset"), a.get("size"), a.get("value_kind")) for a in k["args"]]
            out[k.pop("name")] = k
    return out


def disassembly(co):
    """{symbol: [instruction text, ...]} with addresses, encodings and getpc-relative literals removed."""
    funcs, cur, after_getpc = {}, None, 0
    for line in run(llvm_tool("llvm-objdump"), "-d", "--no-show-raw-insn", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur, after_getpc = funcs.setdefault(m.group(1), []), 0
            continue
        if cur is None or not line.startswith(("\t", " ")):
            continue
        ins = re.sub(r"\s+", " ", line.split("//")[0]).strip()
        if not ins:
            continue
        if after_getpc and re.match(r"s_addc?_u32 ", ins):
            ins = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<pcrel>", ins)
            after_getpc -= 1
        elif ins.startswith("s_getpc_b64"):
            after_getpc = 2
        cur.append(ins)
    for body in funcs.values():  # the padding between functions belongs to nobody
        while body and body[-1].startswith(("s_nop", "s_code_end")):
            body.pop()
    return funcs


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--show", type=int, default=0, help="print the first N differing instructions of each kernel")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        cos = [code_object(lib, a.arch, tmp, tag) for lib, tag in ((a.old, "old"), (a.new, "new"))]
        meta = [metadata(c) for c in cos]
        isa = [disassembly(c) for c in cos]
    names = sorted(set(meta[0]) | set(meta[1]))
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")  # (optional: readable template arguments)
    short = run(filt, *names).splitlines() if filt and names else names
    demangle = {n: re.sub(r"\(.*", "", re.sub(r"^void ", "", s)) for n, s in zip(names, short)}
    bad = 0
    for n in names:
        label = demangle.get(n, n)
        if n not in meta[0] or n not in meta[1]:
            print(f"{'ONLY IN ' + ('old' if n in meta[0] else 'new'):<28} {label}")
            bad += 1
            continue
        mdiff = [f"{k} {meta[0][n].get(k)} -> {meta[1][n].get(k)}" for k in META_FIELDS + ("args",)
                 if meta[0][n].get(k) != meta[1][n].get(k)]
        o, w = isa[0].get(n, []), isa[1].get(n, [])
        same = o == w
        print(f"meta {'equal' if not mdiff else 'DIFF '}  isa {'equal' if same else 'DIFF '} "
              f"({len(o)} -> {len(w)} instructions, {len(w) - len(o):+d})  {label}")
        for d in mdiff:
            print("      " + d)
        if not same and a.show:
            shown = 0
            for i in range(max(len(o), len(w))):
                x, y = (o[i] if i < len(o) else "-"), (w[i] if i < len(w) else "-")
                if x != y:
                    print(f"      [{i}] {x}   |   {y}")
                    shown += 1
                    if shown == a.show:
                        break
        bad += bool(mdiff) or not same
    print(f"{len(names)} kernels, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
