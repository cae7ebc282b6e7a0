#!/usr/bin/env python3
"""Static instruction accounting of one kernel from `hipcc -S` output, per basic block.

usage: python tools/isa_blocks.py <file.s> <kernel name substring> [min MFMA per block]

For every basic block (a run of instructions between labels) of the first kernel whose mangled
name contains every '+'-separated piece of the substring, print the counts DESIGN 4.0.4 uses:
MFMA, other VALU split into address (64-bit adds, shifts-and-adds, mad_u64), select (compares,
v_cndmask, min / max / med3 on integers), move, and the rest; SALU; exec-mask instructions;
branches; LDS reads / writes; global (flat / buffer) loads / stores; s_waitcnt; s_nop; barriers.
The last column counts MFMAs issued directly after the MFMA that wrote their accumulator
(back-to-back dependent issue).  A totals line ends the table, with the kernel's VGPR count and
scratch size.
"""
import re
import sys

ADDR = ("v_lshl_add_u64", "v_mad_u64_u32", "v_mad_i64_i32", "v_lshl_add_u32", "v_add_lshl_u32",
        "v_lshlrev_b64", "v_addc_co_u32", "v_add_co_u32", "v_mad_u32_u24", "v_mul_u32_u24",
        "v_mul_lo_u32", "v_mad_i32_i24", "v_mul_i32_i24", "v_add3_u32", "v_add_u32", "v_sub_u32",
        "v_subrev_u32", "v_lshlrev_b32", "v_lshrrev_b32", "v_ashrrev_i32", "v_and_b32",
        "v_or_b32", "v_and_or_b32", "v_lshl_or_b32", "v_bfe_u32", "v_bfe_i32", "v_xor_b32",
        "v_or3_b32", "v_xad_u32", "v_mul_hi_u32", "v_bfi_b32")
SEL = ("v_cmp", "v_cndmask", "v_min_u32", "v_min_i32", "v_max_u32", "v_max_i32", "v_med3_i32",
       "v_med3_u32", "v_min3", "v_max3")
MOV = ("v_mov_b32", "v_mov_b64", "v_accvgpr", "v_readfirstlane", "v_readlane", "v_writelane")
COLS = ("n", "mfma", "addr", "sel", "mov", "arith", "salu", "exec", "br", "ds_rd", "ds_wr",
        "g_ld", "g_st", "wait", "nop", "bar", "b2b")


def classify(op, args):
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "mfma"
    if op == "s_waitcnt":
        return "wait"
    if op == "s_nop":
        return "nop"
    if op == "s_barrier":
        return "bar"
    if op.startswith("s_cbranch") or op == "s_branch" or op == "s_endpgm" or op == "s_setpc_b64":
        return "br"
    if op.startswith("s_"):
        if "saveexec" in op or re.search(r"\bexec(_lo|_hi)?\b", args.split(",")[0] if args else ""):
            return "exec"
        return "salu"
    if op.startswith("ds_"):
        return "ds_wr" if ("write" in op or "store" in op) else "ds_rd"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "g_st" if ("store" in op or "atomic" in op) else "g_ld"
    if op.startswith("v_"):
        if op.startswith(SEL):
            return "sel"
        if op.startswith(MOV):
            return "mov"
        if op.startswith(ADDR):
            return "addr"
        return "arith"
    return "salu"


def kernel_lines(path, pieces):
    lines = open(path).read().split("\n")
    start = None
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+):", ln)
        if m and all(p in m.group(1) for p in pieces):
            start, name = i, m.group(1)
            break
    if start is None:
        raise SystemExit("no kernel matches %r" % (pieces,))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    meta = {}
    for i, ln in enumerate(lines):
        if ln.strip() == ".name:           " + name or ln.strip() == ".name: " + name or \
                re.match(r"^\s+\.name:\s+%s$" % re.escape(name), ln):
            for l2 in lines[i:i + 40]:
                m = re.match(r"^\s+\.(vgpr_count|private_segment_fixed_size|sgpr_count):\s+(\d+)", l2)
                if m:
                    meta[m.group(1)] = int(m.group(2))
            break
    return name, lines[start + 1:end], meta


def main():
    path, pieces = sys.argv[1], sys.argv[2].split("+")
    min_mfma = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    name, body, meta = kernel_lines(path, pieces)
    blocks, cur, label = [], dict.fromkeys(COLS, 0), "entry"
    last_mfma_dst = None
    loop_of = {}  # block label -> its loop's header label (from the compiler's label comments)
    for ln in body:
        s = ln.split(";")[0].strip()
        if not s or s.startswith("."):
            m = re.match(r"^(\.LBB\w+):", s)
            if m:
                blocks.append((label, cur))
                cur, label, last_mfma_dst = dict.fromkeys(COLS, 0), m.group(1), None
                h = re.search(r"Header=(BB\w+)", ln)
                if "Loop Header" in ln:
                    loop_of[label] = label
                elif h:
                    loop_of[label] = ".L" + h.group(1)
            continue
        parts = s.split(None, 1)
        op, args = parts[0], parts[1] if len(parts) > 1 else ""
        c = classify(op, args)
        cur["n"] += 1
        cur[c] += 1
        if c == "mfma":
            ops = [a.strip() for a in args.split(",")]
            if last_mfma_dst is not None and len(ops) >= 4 and ops[3] == last_mfma_dst:
                cur["b2b"] += 1
            last_mfma_dst = ops[0]
        else:
            last_mfma_dst = None
    blocks.append((label, cur))
    print(name)
    print("%-14s" % "block" + "".join("%7s" % c for c in COLS))
    tot = dict.fromkeys(COLS, 0)
    for lab, b in blocks:
        for c in COLS:
            tot[c] += b[c]
        if b["n"] and b["mfma"] >= min_mfma:
            print("%-14s" % lab + "".join("%7d" % b[c] for c in COLS))
    print("%-14s" % "total" + "".join("%7d" % tot[c] for c in COLS))
    # one pass of every loop: the sum of its blocks (both sides of a branch inside it count)
    loops = {}
    for lab, b in blocks:
        if lab in loop_of:
            s = loops.setdefault(loop_of[lab], dict.fromkeys(COLS, 0))
            for c in COLS:
                s[c] += b[c]
    for h, s in loops.items():
        if s["mfma"] >= min_mfma:
            print("%-14s" % ("loop" + h[4:]) + "".join("%7d" % s[c] for c in COLS))
    print("vgpr %s  sgpr %s  scratch %s" % (meta.get("vgpr_count"), meta.get("sgpr_count"),
                                            meta.get("private_segment_fixed_size")))


if __name__ == "__main__":
    main()
