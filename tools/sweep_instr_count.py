#!/usr/bin/env python3
"""Instruction classes per basic block of one kernel in a gfx950 assembly listing (hipcc -S --cuda-device-only).

    python3 tools/sweep_instr_count.py pgx_mg32.s "k_f_smooth<HIP_vector_type<unsigned int, 2u>, 16, 3, false, 0, 0, 0>"

The kernel is named by a substring of its demangled name (c++filt / llvm-cxxfilt), or of the mangled symbol when neither tool is
there.  Only the blocks that read LDS at least --min-lds-reads times are listed: in the smoother those are the row sweeps (seven
neighbour reads and one store each) and the residual rows of the restriction epilogue.  The script looks at mnemonics only - which
unit an instruction issues to - and at the kernel's resource lines; it does not interpret operands.
"""
import argparse
import re
import shutil
import subprocess
import sys


def demangle(names):
    for tool in ("c++filt", "llvm-cxxfilt", "/opt/rocm/llvm/bin/llvm-cxxfilt"):
        exe = shutil.which(tool)
        if exe:
            out = subprocess.run([exe], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
    return {n: n for n in names}


def classify(mn):
    """-> one of valu, salu, lds_read, lds_write, vmem, other"""
    if mn.startswith("ds_"):
        return "lds_write" if "write" in mn or "store" in mn else "lds_read"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith("s_"):
        if mn.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_cbranch", "s_branch", "s_endpgm", "s_load", "s_buffer_load", "s_sleep",
                          "s_setprio", "s_code_end")):
            return "other"
        return "salu"
    return "other"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("kernel", help="substring of the demangled (or mangled) kernel name")
    ap.add_argument("--min-lds-reads", type=int, default=4)
    ap.add_argument("--all-blocks", action="store_true")
    a = ap.parse_args()

    lines = open(a.asm).read().split("\n")
    starts = {}  # symbol -> line index of "symbol:"
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$", ln)
        if m and not m.group(1).startswith(".L"):
            starts[m.group(1)] = i
    names = demangle(list(starts))
    hits = [s for s in starts if a.kernel in names[s] or a.kernel in s]
    if len(hits) != 1:
        sys.exit(f"{len(hits)} kernels match {a.kernel!r}:\n  " + "\n  ".join(names[s] for s in hits[:40]))
    sym = hits[0]
    print(f"kernel {names[sym]}")

    blocks, cur = [], None
    end = len(lines)
    for i in range(starts[sym] + 1, len(lines)):
        ln = lines[i].strip()
        if ln.startswith(".Lfunc_end"):
            end = i
            break
        m = re.match(r"^(\.LBB\w+):", ln)
        if m or cur is None:
            cur = {"label": m.group(1) if m else "entry", "n": {}, "pk": 0, "mov": 0, "read2": 0}
            blocks.append(cur)
            if m:
                continue
        if not ln or ln.startswith((";", ".", "//")):
            continue
        mn = ln.split()[0]
        c = classify(mn)
        cur["n"][c] = cur["n"].get(c, 0) + 1
        cur["pk"] += mn.startswith("v_pk_")
        cur["mov"] += mn in ("v_mov_b32_e32", "v_mov_b32", "v_mov_b64", "v_mov_b64_e32", "v_accvgpr_read_b32", "v_accvgpr_write_b32")
        cur["read2"] += mn.startswith("ds_read2")

    print(f"{'block':>12} {'VALU':>5} {'v_pk':>5} {'v_mov':>5} {'SALU':>5} {'LDSrd':>5} {'read2':>5} {'LDSwr':>5} {'VMEM':>5}")
    shown = 0
    for b in blocks:
        n = b["n"]
        if not a.all_blocks and n.get("lds_read", 0) < a.min_lds_reads:
            continue
        shown += 1
        print(f"{b['label']:>12} {n.get('valu', 0):5d} {b['pk']:5d} {b['mov']:5d} {n.get('salu', 0):5d} {n.get('lds_read', 0):5d} "
              f"{b['read2']:5d} {n.get('lds_write', 0):5d} {n.get('vmem', 0):5d}")
    print(f"{shown} of {len(blocks)} blocks listed")
    # the kernel's resource usage as the assembler comments state it
    for i in range(end, min(end + 400, len(lines))):
        m = re.match(r"^\s*;\s*(NumVgprs|NumAgprs|ScratchSize|Occupancy|SGPRBlocks|NumSgprs|LDSByteSize|TotalNumVgprs)\b.*", lines[i])
        if m:
            print(lines[i].strip().lstrip("; "))
        if lines[i].strip().startswith(".Lfunc_end") and i > end:
            break


if __name__ == "__main__":
    main()
