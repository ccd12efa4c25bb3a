"""Instruction mix of the MFMA loops in hipcc's gfx950 assembly of a .hip file: per kernel and per
basic block that contains MFMAs, the counts of MFMA, other VALU, SALU, s_waitcnt, ds_read,
ds_write and global-load instructions, and whether the block branches to itself (a steady loop
body). Opcode classes only: compile-time evidence of what a loop issues next to its MFMAs, not a
measurement. CPU only (hipcc cross-compile).

  python tools/loop_mix.py csrc/hip/conv_wino.hip [kernel-name-substring ...]

A `v_mfma_f32_16x16x32_bf16` holds the SIMD's vector issue for 8 of its 16 matrix-pipe cycles and
a plain VALU instruction for 4, so at r VALU per MFMA the issue time per MFMA slot is 8 + 4 r
cycles: above the pipe's 16 from r = 2.0 (docs/KERNELS.md, 'Winograd loop: VALU per MFMA').
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("mfma", "valu", "salu", "waitcnt", "ds_read", "ds_write", "gload")


def assembly(src):
    """(assembly text, demangled-name lookup) of `src` compiled for gfx950 like the build does."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "x.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                        "-munsafe-fp-atomics", "-Wno-unused-result", "--cuda-device-only", "-S",
                        "-I" + os.path.join(ROOT, "csrc", "hip"), os.path.abspath(src), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read()


def demangle(names):
    """Demangled names where a demangler is installed (the mangled ones otherwise)."""
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    try:
        res = subprocess.run([filt] + list(names), check=True, capture_output=True, text=True)
        lines = res.stdout.splitlines()
        if len(lines) == len(names):
            return dict(zip(names, lines))
    except (OSError, TypeError, subprocess.CalledProcessError):
        pass
    return {n: n for n in names}


def classify(op):
    if op.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if op == "s_waitcnt":
        return "waitcnt"
    if op.startswith("ds_read") or op.startswith("ds_load"):
        return "ds_read"
    if op.startswith("ds_write") or op.startswith("ds_store"):
        return "ds_write"
    if op.startswith(("buffer_load", "global_load", "flat_load", "scratch_load")):
        return "gload"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_") and not op.startswith(("s_nop", "s_barrier", "s_cbranch", "s_branch",
                                                  "s_endpgm", "s_sleep", "s_setprio")):
        return "salu"
    return None


def kernels(asm):
    """{mangled kernel: {"scratch": bytes, "vgprs": n, "blocks": [block dict in order]}} where a
    block dict has the FIELDS counts, "label" and "self_loop"; MFMA-free blocks are left out."""
    out = {}
    name, blk = None, None
    for line in asm.split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = {"scratch": None, "vgprs": None, "blocks": []}
            blk = dict.fromkeys(FIELDS, 0) | {"label": "entry", "self_loop": False}
            out[name]["blocks"].append(blk)
            continue
        if name is None:
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m:
            blk = dict.fromkeys(FIELDS, 0) | {"label": m.group(1), "self_loop": False}
            out[name]["blocks"].append(blk)
            continue
        m = re.match(r"^\s*; ScratchSize: (\d+)", line)
        if m:
            out[name]["scratch"] = int(m.group(1))
            continue
        m = re.match(r"^\s*; NumVgprs: (\d+)", line)
        if m:
            out[name]["vgprs"] = int(m.group(1))
            continue
        if line.startswith(".Lfunc_end"):
            blk = None
            continue
        m = re.match(r"^\s+([a-z_][a-z0-9_]*)\s*(.*)$", line)
        if not m or blk is None:
            continue
        op, args = m.group(1), m.group(2)
        if op.startswith(("s_cbranch", "s_branch")) and args.split()[0:1] == [blk["label"]]:
            blk["self_loop"] = True
        c = classify(op)
        if c:
            blk[c] += 1
    for k in out.values():
        k["blocks"] = [b for b in k["blocks"] if b["mfma"]]
    return {n: k for n, k in out.items() if k["scratch"] is not None}


def report(src, want=()):
    ks = kernels(assembly(src))
    names = demangle(list(ks))
    rows = []
    for n, k in ks.items():
        nice = names[n].replace("(anonymous namespace)::", "")
        nice = re.sub(r"^void ", "", nice).split("(")[0]
        if not k["blocks"] or (want and not any(w in nice for w in want)):
            continue
        rows.append((nice, k))
    return rows


def main(argv):
    if not argv:
        print(__doc__)
        return 2
    for nice, k in report(argv[0], argv[1:]):
        print("%s  vgprs %s  scratch %s B" % (nice, k["vgprs"], k["scratch"]))
        print("    %-12s %5s %5s %5s %5s %5s %5s %5s  %9s  %s" %
              (("block",) + tuple(f[:5] for f in FIELDS) + ("valu/mfma", "self-loop")))
        for b in k["blocks"]:
            print("    %-12s %5d %5d %5d %5d %5d %5d %5d  %9.2f  %s" %
                  ((b["label"],) + tuple(b[f] for f in FIELDS) +
                   (b["valu"] / b["mfma"], "yes" if b["self_loop"] else "")))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
