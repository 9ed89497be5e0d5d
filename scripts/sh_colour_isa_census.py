"""Static census of the deferred colour kernels' trips to memory, from the compiler's own assembly (no GPU needed): the sibling
of kernel_isa_census.py for a kernel whose cost is how its loads are ordered rather than how many instructions it has.

Per kernel: VGPRs, scratch bytes and occupancy from the kernel's footer, and for every EVALUATION REGION -- a stretch of the
kernel from a block that loads a 12- or 16-byte piece to the 12-byte store of the colour -- the global loads by width and the
number of DEPENDENT TRIPS: bursts of loads separated by an ``s_waitcnt vmcnt`` (a load issued after a wait cannot have been in
flight with the loads before it; partial waits on one burst, vmcnt(11) .. vmcnt(0), are one trip).  The coefficient-by-
coefficient path is one region of four trips (the degree tests sit between the bursts); the record path is one region of one.
    python scripts/sh_colour_isa_census.py [--markdown] [--tree DIR]
DIR is another checkout of this repository (its csrc is compiled with this checkout's flags), for a before / after.
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from autovfx_amd import build  # noqa: E402
from kernel_isa_census import assembly  # noqa: E402

KERNELS = [("sh_colour_listed_kernel", "sh_colour_listed_kernel"), ("sh_colour_all_kernel", "sh_colour_all_kernel")]
WIDE = ("global_load_dwordx3", "global_load_dwordx4")


def kernel_lines(lines, part):
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and part in l and l.split(";")[0].rstrip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".amdhsa_kernel"))
    foot = {}
    for l in lines[end:]:
        m = re.match(r";\s*(NumVgprs|ScratchSize|Occupancy):\s*(\d+)", l)
        if m:
            foot[m.group(1)] = int(m.group(2))
            if len(foot) == 3:
                break
    ops = []
    for l in lines[start + 1:end]:
        s = l.split(";")[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            ops.append(s)
            if s.split()[0] == "s_endpgm":
                break
    return ops, foot


def regions(ops):
    """[(loads by width, trips)] of every evaluation region, in program order."""
    out, cur = [], None
    for s in ops:
        op = s.split()[0]
        # A region opens at a wide load at offset 0 of its own address (the position, or piece 0 of a record).  The block layout
        # may put a loop's store before its loads, so a region also ends where the next one opens: at a load behind a wait whose
        # offset is below one already seen (within a region the offsets only ascend from burst to burst).  Where the compiler
        # hoists the position load above the test that picks the path, it is counted with the first region.
        m = re.search(r"offset:(\d+)", s)
        off = int(m.group(1)) if m else 0
        opens = op in WIDE and ((cur is None and m is None) or (cur is not None and cur["waited"] and off < cur["max_off"]))
        if opens or (cur is not None and op.startswith("global_load_")):
            if opens:
                if cur is not None:
                    out.append((cur["loads"], cur["trips"]))
                cur = {"loads": {}, "trips": 0, "waited": True, "max_off": 0}
            cur["max_off"] = max(cur["max_off"], off)
            if cur["waited"]:
                cur["trips"] += 1
                cur["waited"] = False
            cur["loads"][op] = cur["loads"].get(op, 0) + 1
        elif cur is not None and op == "s_waitcnt" and "vmcnt" in s:
            cur["waited"] = True
        elif cur is not None and op == "global_store_dwordx3":
            out.append((cur["loads"], cur["trips"]))
            cur = None
        elif cur is not None and op == "global_store_dwordx4":   # (the ranges duty copies 16-byte pieces: not an evaluation)
            cur = None
    if cur is not None:   # a loop laid out with its store first
        out.append((cur["loads"], cur["trips"]))
    return out


def main():
    csrc = build.CSRC
    if "--tree" in sys.argv:
        csrc = os.path.join(os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]), "autovfx_amd", "csrc")
    lines = assembly(csrc, "gsr_kernels.hip")
    md = "--markdown" in sys.argv
    if md:
        print("| kernel | VGPRs | scratch | occupancy | region | dword | dwordx2 | dwordx3 | dwordx4 | dependent trips |")
        print("|---|---|---|---|---|---|---|---|---|---|")
    for part, name in KERNELS:
        ops, foot = kernel_lines(lines, part)
        for n, (loads, trips) in enumerate(regions(ops)):
            w = [loads.get("global_load_dword" + x, 0) for x in ("", "x2", "x3", "x4")]
            if md:
                print(f"| `{name}` | {foot.get('NumVgprs')} | {foot.get('ScratchSize')} | {foot.get('Occupancy')} | {n} | "
                      + " | ".join(str(v) for v in w) + f" | {trips} |")
            else:
                print(f"{name:24s} vgpr={foot.get('NumVgprs')} scratch={foot.get('ScratchSize')} occupancy={foot.get('Occupancy')} "
                      f"region {n}: dword={w[0]} x2={w[1]} x3={w[2]} x4={w[3]} trips={trips}")


if __name__ == "__main__":
    main()
