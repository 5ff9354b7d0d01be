#!/usr/bin/env python3
"""Registers, spills and LDS of every k_gp_tile instantiation in a built libgpmdm_hip.so (CPU
only: reads the code objects' metadata with ROCm's llvm-readelf).

    python tools/tile_resources.py [LIB] [--against OTHER_LIB] [--md]

One row per instantiation <d, dyn, flags, NW, MT, NTW>: VGPRs, spilled VGPRs, scratch bytes per
lane, SGPRs, LDS bytes per workgroup.  With --against, OTHER_LIB's figures stand beside them
(before -> after), so a change to gp_tile.h can be judged before any GPU time."""
import argparse
import re
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
LLVM = Path("/opt/rocm/llvm/bin")
TILE = re.compile(r"k_gp_tileILi(\d+)ELb([01])ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E")
KEYS = (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".sgpr_count", ".group_segment_fixed_size")


def code_objects(lib: Path, tmp: Path):
    fat = tmp / "fat.bin"
    subprocess.run([str(LLVM / "llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", str(lib), str(tmp / "x.o")],
                   check=True, capture_output=True)
    b = fat.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out, pos = [], 0
    while (i := b.find(magic, pos)) >= 0:
        n = struct.unpack_from("<Q", b, i + 24)[0]
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", b, p)
            p += 24
            triple = b[p:p + tl].decode()
            p += tl
            if triple.endswith("gfx950") and size:
                co = tmp / f"co{len(out)}.o"
                co.write_bytes(b[i + off:i + off + size])
                out.append(co)
        pos = i + 1
    return out


def tile_table(lib: Path) -> dict:
    table = {}
    with tempfile.TemporaryDirectory() as t:
        for co in code_objects(lib, Path(t)):
            notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True,
                                   text=True).stdout
            for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", block)
                m = name and TILE.search(name.group(1))
                if not m:
                    continue
                row = []
                for k in KEYS:
                    v = re.search(re.escape(k) + r":\s+(\d+)", block)
                    row.append(int(v.group(1)) if v else 0)
                table[tuple(int(x) for x in m.groups())] = tuple(row)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib", nargs="?", default=str(ROOT / "gpmdm_amd" / "libgpmdm_hip.so"))
    ap.add_argument("--against", default=None, help="a second library (e.g. the parent commit's build): before -> after")
    ap.add_argument("--md", action="store_true", help="a markdown table")
    args = ap.parse_args()
    new = tile_table(Path(args.lib))
    old = tile_table(Path(args.against)) if args.against else None
    if not new:
        sys.exit("no k_gp_tile kernel found")
    head = ["d", "dyn", "flags", "NW", "MT", "NTW", "VGPR", "spilled", "scratch B", "SGPR", "LDS B"]
    sep = " | " if args.md else "  "
    lines = [sep.join(head)]
    if args.md:
        lines.append(sep.join("---" for _ in head))
    for key in sorted(new):
        cells = [str(x) for x in key]
        for i, v in enumerate(new[key]):
            o = old.get(key) if old else None
            cells.append(f"{o[i]} -> {v}" if o is not None and o[i] != v else str(v))
        lines.append(sep.join(cells))
    print("\n".join(("| " + ln + " |") if args.md else ln for ln in lines))


if __name__ == "__main__":
    main()
