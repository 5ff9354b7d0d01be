#!/usr/bin/env python3
"""Instruction mix of the K-step loop bodies of a built tile kernel (CPU only: reads assembly).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude --cuda-device-only -S \\
        gpmdm_amd/csrc/gp_tile_d1.hip -o d1.s
    python tools/tile_kstep_mix.py d1.s --kernel k_gp_tileILi3ELb0ELi0ELi4ELi2ELi8E [--md]

The input is compiler assembly (``-S``) or ``llvm-objdump -d --symbolize-operands`` of a code
object.  A K-step loop body is an innermost loop (a label up to a branch back to it) that holds
MFMAs: k_gp_tile has one per phase [T0, T1) of retired column tiles.  For each body, in program
order over all its basic blocks (the fragments' branches included):

* the counts of MFMA, other VALU, SALU, DS, buffer, ``s_waitcnt`` and branch instructions;
* how many VALU and SALU stand before the first MFMA (the head) and after the last (the tail).

Instructions are classified by mnemonic prefix only: ``v_mfma``; other ``v_``; ``s_waitcnt``;
``s_cbranch`` / ``s_branch``; other ``s_``; ``ds_``; ``buffer_``.  Everything else is "other"."""
import argparse
import re
import sys

LABEL = re.compile(r"^\s*<?(\.?L[A-Za-z_]*\d+(?:_\d+)?)>?:")
FUNC = re.compile(r"^(?:[0-9a-f]+ <)?([A-Za-z_][\w.$]*)>?:\s*(?:;.*)?$")
BRANCH = re.compile(r"^(s_cbranch_\w+|s_branch)\s+<?(\.?L[A-Za-z_]*\d+(?:_\d+)?)>?")
CLASSES = ("mfma", "valu", "salu", "ds", "buffer", "waitcnt", "branch", "other")


def classify(mn: str) -> str:
    if mn.startswith("v_mfma"):
        return "mfma"
    if mn.startswith("v_"):
        return "valu"
    if mn.startswith("s_waitcnt"):
        return "waitcnt"
    if mn.startswith("s_cbranch") or mn.startswith("s_branch"):
        return "branch"
    if mn.startswith("s_"):
        return "salu"
    if mn.startswith("ds_"):
        return "ds"
    if mn.startswith("buffer_"):
        return "buffer"
    return "other"


def kernels(text: str):
    """{name: [lines]}: the text split at function labels (mangled names)."""
    out, name = {}, None
    for raw in text.splitlines():
        line = raw.split(";")[0].split("//")[0].rstrip()
        m = FUNC.match(raw.strip()) if not raw.startswith((" ", "\t")) or "<" in raw[:20] else None
        if m and not LABEL.match(raw) and (m.group(1).startswith("_Z") or "k_" in m.group(1)):
            name = m.group(1)
            out[name] = []
            continue
        if name is not None:
            out[name].append(line)
    return out


def instructions(lines):
    """[(label or None, mnemonic, branch target or None)] in program order."""
    seq = []
    for line in lines:
        lm = LABEL.match(line)
        if lm:
            seq.append((lm.group(1), None, None))
            continue
        s = line.strip()
        s = re.sub(r"^[0-9a-f]+:\s+", "", s)                  # objdump's address column, if any
        if not s or s.startswith("."):
            continue
        mn = s.split()[0]
        if not re.match(r"^[a-z][a-z0-9_]*$", mn):
            continue
        bm = BRANCH.match(s)
        seq.append((None, mn, bm.group(2) if bm else None))
    return seq


def kstep_loops(seq):
    """[(label, first, last)]: innermost loops holding MFMAs, by index into ``seq``."""
    at = {lab: i for i, (lab, _, _) in enumerate(seq) if lab}
    loops = [(at[t], i, t) for i, (_, mn, t) in enumerate(seq) if t in at and at[t] < i]
    with_mfma = [(a, b, t) for a, b, t in loops if any(m and m.startswith("v_mfma") for _, m, _ in seq[a:b + 1])]
    inner = [x for x in with_mfma if not any(y is not x and x[0] <= y[0] and y[1] <= x[1] for y in with_mfma)]
    return [(t, a, b) for a, b, t in sorted(inner)]


def mix(seq, a, b):
    body = [mn for _, mn, _ in seq[a:b + 1] if mn]
    cls = [classify(mn) for mn in body]
    row = {c: cls.count(c) for c in CLASSES}
    mf = [i for i, c in enumerate(cls) if c == "mfma"]
    head, tail = cls[:mf[0]], cls[mf[-1] + 1:]
    row.update(head_valu=head.count("valu"), head_salu=head.count("salu"), tail_valu=tail.count("valu"),
               tail_salu=tail.count("salu"))
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", help="assembly of the kernel (hipcc -S, or llvm-objdump -d --symbolize-operands)")
    ap.add_argument("--kernel", default="k_gp_tile", help="substring of the (mangled) kernel name")
    ap.add_argument("--md", action="store_true", help="a markdown table")
    args = ap.parse_args()
    ks = {n: ls for n, ls in kernels(open(args.asm).read()).items() if args.kernel in n}
    if not ks:
        sys.exit(f"no kernel matching {args.kernel!r}")
    cols = ["mfma", "valu", "salu", "ds", "buffer", "waitcnt", "branch", "head_valu", "head_salu", "tail_valu", "tail_salu"]
    sep = " | " if args.md else "  "
    for name, lines in ks.items():
        seq = instructions(lines)
        loops = kstep_loops(seq)
        print(("### " if args.md else "== ") + f"{name}: {len(loops)} K-step loop bodies")
        out = [sep.join(["loop"] + cols)]
        if args.md:
            out.append(sep.join("---" for _ in range(len(cols) + 1)))
        for lab, a, b in loops:
            r = mix(seq, a, b)
            out.append(sep.join([lab] + [str(r[c]) for c in cols]))
        print("\n".join(("| " + ln + " |") if args.md else ln for ln in out))


if __name__ == "__main__":
    main()
