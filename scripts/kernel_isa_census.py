"""Static instruction census of whole kernels from the compiler's own assembly (no GPU needed): the sibling of
blend_isa_census.py for kernels whose cost is their instruction count from top to bottom rather than one inner loop.

Compiles a unit of autovfx_amd/csrc with the library's flags to gfx950 assembly and prints, per kernel, the number of
vector instructions (and of the kinds the projection kernel was trimmed for: moves, selects, compares, cross-lane
moves, division and square-root pieces), scalar, LDS and memory instructions, and the register / LDS figures of the
kernel descriptor.
    python scripts/kernel_isa_census.py [--markdown] [--tree DIR] [--units UNIT.hip ...]
DIR is another checkout of this repository (its csrc is compiled with this checkout's flags), for a before / after.
--units: every kernel of the named units instead of the three of the table below.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autovfx_amd import build  # noqa: E402

KERNELS = [("gsr_kernels.hip", "preprocess_kernelILb0", "preprocess_kernel<false>"),
           ("gsr_kernels.hip", "preprocess_kernelILb1", "preprocess_kernel<true>"),
           ("gsr_binning.hip", "expand_kernel", "expand_kernel")]
COLS = ["VALU", "v_mov", "v_cndmask", "v_cmp", "dpp", "ds_bpermute", "v_div_*", "v_rcp", "v_sqrt", "SALU", "LDS", "VMEM",
        "vgpr", "sgpr", "lds_bytes", "scratch"]


def assembly(csrc, unit):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "unit.s")
        flags = [f for f in build.FLAGS if f not in ("-fPIC",)]
        subprocess.check_call([build.hipcc(), "-x", "hip", *flags, "--cuda-device-only", "-S", "-o", out,
                               os.path.join(csrc, unit)], stderr=subprocess.DEVNULL)
        return open(out).read().splitlines()


def census(lines, mangled_part):
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and mangled_part in l and l.split(";")[0].rstrip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".amdhsa_kernel"))
    stop = next(i for i in range(end, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
    c = dict.fromkeys(COLS, 0)
    for l in lines[start:end]:
        s = l.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        op = s.split()[0]
        if op == "s_endpgm":
            break
        if op.startswith("v_"):
            c["VALU"] += 1
            if re.search(r"\b(row_shr|row_bcast|row_shl|quad_perm|wave_shr|row_ror)", s) or op.endswith("_dpp"):
                c["dpp"] += 1
            for k, pre in (("v_mov", "v_mov_b32"), ("v_cndmask", "v_cndmask"), ("v_cmp", "v_cmp"), ("v_div_*", "v_div_"),
                           ("v_rcp", "v_rcp"), ("v_sqrt", "v_sqrt")):
                if op.startswith(pre):
                    c[k] += 1
        elif op.startswith("ds_"):
            c["LDS"] += 1
            if op.startswith("ds_bpermute"):
                c["ds_bpermute"] += 1
        elif op.startswith("s_"):
            c["SALU"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["VMEM"] += 1
    for l in lines[end:stop]:
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|group_segment_fixed_size|private_segment_fixed_size)\s+(\d+)", l)
        if m:
            c[{"next_free_vgpr": "vgpr", "next_free_sgpr": "sgpr", "group_segment_fixed_size": "lds_bytes",
               "private_segment_fixed_size": "scratch"}[m.group(1)]] = int(m.group(2))
    return c


def main():
    csrc = build.CSRC
    if "--tree" in sys.argv:
        csrc = os.path.join(os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]), "autovfx_amd", "csrc")
    units = {}
    rows = []
    kernels = KERNELS
    if "--units" in sys.argv:   # every kernel the unit's assembly declares, under its mangled name
        kernels = []
        for unit in sys.argv[sys.argv.index("--units") + 1:]:
            if unit.startswith("--"):
                break
            units[unit] = assembly(csrc, unit)
            names = [l.split()[1] for l in units[unit] if l.strip().startswith(".amdhsa_kernel ")]
            kernels += [(unit, n + ":", unit[:-4] + " " + re.sub(r"^_ZN3gsr(\d+_GLOBAL__N_1)?\d+", "", n)[:48]) for n in names]
    for unit, part, name in kernels:
        if unit not in units:
            units[unit] = assembly(csrc, unit)
        rows.append((name, census(units[unit], part)))
    if "--markdown" in sys.argv:
        print("| kernel | " + " | ".join(COLS) + " |")
        print("|---|" + "---|" * len(COLS))
        for name, c in rows:
            print(f"| `{name}` | " + " | ".join(str(c[k]) for k in COLS) + " |")
    else:
        for name, c in rows:
            print((f"{name:26s} " if kernels is KERNELS else f"{name:64s} ") + "  ".join(f"{k}={c[k]}" for k in COLS))


if __name__ == "__main__":
    main()
