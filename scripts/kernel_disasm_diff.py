"""Do two source trees compile to the same GPU code?  Compiles every .hip file of opencl_render_amd/csrc in both trees for gfx950 (device
code only, the Makefile's DEVFLAGS), disassembles the code objects with llvm-objdump and compares them symbol by symbol (kernels and the device functions not inlined).  The address
comments llvm-objdump prints are dropped, and so is the padding (s_nop, zero bytes) after a kernel's s_endpgm (it depends on where the next symbol
starts); the instruction text, relative branch offsets included, is compared.  Needs no GPU.

    python scripts/kernel_disasm_diff.py --base /path/to/parent/checkout [--new .] [--keep DIR]

Prints per source file the symbols that are identical, changed, moved, removed and added, and exits 1 if any existing symbol changed or
went.  Symbols are matched over all files together: one that left its file and is new in another has moved, and passes if its instructions
are the same.  The last line printed is the verdict.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("rt_kernels", "rt_wavefront", "rt_scene_passes", "rt_build_device", "rt_kat", "rt_scene_prep", "rt_denoise", "rt_temporal", "rt_variance",
           "rt_camera_move", "rt_geometry_move", "rt_scene_edit", "rt_motion_blur", "rt_dof")


def devflags(tree):
    text = open(os.path.join(tree, "opencl_render_amd", "csrc", "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^DEVFLAGS\s*:=(.*)$", text, re.M)
    return m.group(1).replace("$(ARCH)", "gfx950").split()


def disassemble(tree, out, rocm):
    csrc = os.path.join(tree, "opencl_render_amd", "csrc")
    kernels = {}
    for name in SOURCES:
        if not os.path.exists(os.path.join(csrc, name + ".hip")):  # a file one tree does not have yet: every symbol of it is added or gone
            kernels[name] = {}
            continue
        co = os.path.join(out, name + ".co")
        subprocess.run([os.path.join(rocm, "bin", "hipcc")] + devflags(tree) + ["-I" + os.path.join(tree, "include"), "-I" + csrc,
                       "--cuda-device-only", "--no-gpu-bundle-output", "-c", os.path.join(csrc, name + ".hip"), "-o", co], check=True)
        dis = subprocess.run([os.path.join(rocm, "llvm", "bin", "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                             check=True, capture_output=True, text=True).stdout
        body, cur = {}, None
        for line in dis.splitlines():
            m = re.match(r"^<(.+)>:$", line.strip())
            if m:
                cur = m.group(1)
                body[cur] = []
            elif cur is not None and line.strip():
                body[cur].append(re.sub(r"\s*//.*$", "", line).strip())
        for insns in body.values():  # the padding up to the next symbol's alignment (s_nop, zero bytes: "...") is not the function's code
            while insns and insns[-1] in ("s_nop 0", "...") and "s_endpgm" in insns:
                insns.pop()
        kernels[name] = body
    return kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True, help="root of the tree to compare against (e.g. a checkout of the parent commit)")
    ap.add_argument("--new", default=ROOT, help="root of the tree under review (default: this one)")
    ap.add_argument("--keep", help="keep the code objects here (default: a temporary directory)")
    ap.add_argument("--rocm", default=os.environ.get("ROCM_PATH", "/opt/rocm"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        keep = args.keep or tmp
        os.makedirs(os.path.join(keep, "base"), exist_ok=True)
        os.makedirs(os.path.join(keep, "new"), exist_ok=True)
        a = disassemble(args.base, os.path.join(keep, "base"), args.rocm)
        b = disassemble(args.new, os.path.join(keep, "new"), args.rocm)
    # A symbol that left its file and is new in another one is the same symbol, moved.  home[(file, symbol)]: the file it went to.
    home = {}
    for name in SOURCES:
        for k in a[name]:
            if k not in b[name]:
                for other in SOURCES:
                    if other != name and k in b[other] and k not in a[other]:
                        home[(name, k)] = other
                        break
    arrived = {name: [k for (_, k), to in home.items() if to == name] for name in SOURCES}
    bad = False
    for name in SOURCES:
        ka, kb = a[name], b[name]
        after = {k: b[home.get((name, k), name)].get(k) for k in ka}  # each old symbol's instructions now, wherever it lives; None: gone
        same = [k for k in ka if k in kb and after[k] == ka[k]]
        moved = [k for k in ka if k not in kb and after[k] == ka[k]]
        changed = [k for k in ka if after[k] is not None and after[k] != ka[k]]
        gone = [k for k in ka if after[k] is None]
        added = [k for k in kb if k not in ka and k not in arrived[name]]
        print(f"{name}.hip: {len(ka)} symbols before, {len(kb)} after: {len(same)} identical, {len(changed)} changed, "
              f"{len(moved)} moved, {len(gone)} removed, {len(added)} added, {len(arrived[name])} moved in")
        for k in changed:
            where = f", now in {home[(name, k)]}.hip" if (name, k) in home else ""
            print(f"  changed  {k}{where} ({len(ka[k])} -> {len(after[k])} instructions)")
        for k in moved:
            print(f"  moved    {k} to {home[(name, k)]}.hip, identical ({len(ka[k])} instructions)")
        for k in gone:
            print(f"  removed  {k}")
        for k in added:
            print(f"  added    {k} ({len(kb[k])} instructions)")
        bad = bad or bool(changed or gone)
    print("FAIL: an existing symbol changed or went" if bad else "OK: every existing symbol is identical, in its file or moved")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
