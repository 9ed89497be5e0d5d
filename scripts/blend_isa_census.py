"""Instruction census of blend_quadrant_kernel's inner loop from the compiler's own assembly (no GPU needed).

Compiles autovfx_amd/csrc/gsr_blend.hip with the library's flags to gfx950 assembly, finds the innermost loop of
blend_quadrant_kernel<false> (the walk over the staged entries that reach the quadrant: the loop that holds the
v_exp_f32) and splits every entry of its body -- the body is unrolled over several LDS slots, one entry each -- into
the stages an entry can stop at:
    A  every processed entry : slot reads, power, the two range tests (plus the loop's own address arithmetic,
                               which is spread over the entries of the body)
    B  some pixel in range   : exp, alpha, the 1/255 test
    C  some pixel blends     : T (1 - alpha), the 1e-4 test
    D  some pixel accumulates: colour read, the four packed multiply-adds, T and last-contributor update, and the
                               bound check that leads to the next slot / the loop tail
and prints per stage VALU (of which comparisons / transcendental / packed), SALU, LDS and wait instructions, averaged
over the entries of the body.
    python scripts/blend_isa_census.py [--markdown] [--extra] [--tree DIR] [--dump] [--staging]
--extra: blend_quadrant_kernel<true>.  DIR is another checkout of this repository (its csrc is compiled with this
checkout's flags), for a before / after.  --staging: the per-batch staging block of both kernels instead (staging_census).
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autovfx_amd import build  # noqa: E402

STAGES = ["A every processed entry", "B some pixel in range", "C some pixel blends", "D accumulate + next slot"]
KINDS = ["valu", "v_cmp", "trans", "v_pk", "salu", "branch", "lds", "wait", "vmem", "other"]
COLS = ["VALU total", "valu", "v_cmp", "trans", "v_pk", "SALU total", "lds", "wait", "vmem"]


def assembly(csrc=None):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "blend.s")
        flags = [f for f in build.FLAGS if f not in ("-fPIC",)]
        subprocess.check_call([build.hipcc(), "-x", "hip", *flags, "--cuda-device-only", "-S", "-o", out,
                               os.path.join(csrc or build.CSRC, "gsr_blend.hip")], stderr=subprocess.DEVNULL)
        return open(out).read()


def kernel_body(asm, mangled_part="blend_quadrant_kernelILb0"):
    lines = asm.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and mangled_part in l and l.split(";")[0].rstrip().endswith(":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".amdhsa_kernel"))
    return lines[start:end]


def classify(op):
    if op.startswith(("v_cmp", "v_cmpx")):
        return "v_cmp"
    if op.startswith(("v_exp", "v_log", "v_rcp", "v_rsq", "v_sqrt", "v_sin", "v_cos")):
        return "trans"
    if op.startswith("v_pk_"):
        return "v_pk"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "other"


def walk_loop(body):
    """The lines of the innermost loop that evaluates entries: from its header label to the backward branch to it."""
    for hdr in (i for i, l in enumerate(body) if "Inner Loop Header" in l):
        label = next(m.group(1) for m in (re.match(r"^(\.LBB\d+_\d+):", body[j]) for j in range(hdr, -1, -1)) if m)
        first = next(i for i, l in enumerate(body) if l.startswith(label + ":"))
        back = [i for i, l in enumerate(body) if i > first and re.search(r"s_c?branch\w*\s+" + re.escape(label) + r"\b", l)]
        if back and any("v_exp_f32" in l for l in body[first:max(back) + 1]):
            return body[first:max(back) + 1]
    raise RuntimeError("no inner loop with a v_exp_f32 in the kernel")


def instructions(loop):
    out = []
    for l in loop:
        s = l.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            out.append(("label", m.group(1)))
        elif s and not s.startswith((";", ".", "//")):
            out.append((classify(s.split()[0]), s))
    return out


def entries(loop):
    """One list of four stages per entry of the (unrolled) body.  Stages A to C end at the conditional branch that follows a
    comparison (the early exits); the entry ends at the first branch at or behind the label its first early exit jumps to (the
    next slot's bound check), or with the loop."""
    ins, out, i = instructions(loop), [], 0
    while i < len(ins):
        stages, cur, skip_to, seen = [], [], None, False
        while i < len(ins):
            kind, text = ins[i]
            i += 1
            cur.append((kind, text))
            if kind == "label" and text == skip_to:
                seen = True
            if kind != "branch":
                continue
            if len(stages) < 3 and text.startswith("s_cbranch") and any(k == "v_cmp" for k, _ in cur):
                if not stages:
                    skip_to = text.split()[-1]
                stages.append(cur)
                cur = []
            elif len(stages) == 3 and seen:
                break
        stages.append(cur)
        if len(stages) == 4:
            out.append(stages)
        elif out:   # what follows the last entry (the loop's tail) belongs to its last stage
            out[-1][-1].extend(c for st in stages for c in st)
    return out


def stage_table(mangled_part="blend_quadrant_kernelILb0", csrc=None):
    """(number of entries in the loop body, [per stage: {column: count averaged over the entries}])."""
    ent = entries(walk_loop(kernel_body(assembly(csrc), mangled_part)))
    rows = []
    for k in range(4):
        cnt = {c: sum(1 for st in ent for kind, _ in st[k] if kind == c) / len(ent) for c in KINDS}
        cnt["VALU total"] = cnt["valu"] + cnt["v_cmp"] + cnt["trans"] + cnt["v_pk"]
        cnt["SALU total"] = cnt["salu"] + cnt["branch"]
        rows.append(cnt)
    return len(ent), rows


def staging_census(asm, mangled_part="blend_quadrant_kernelILb0"):
    """What a batch of 64 list entries costs before its walk starts: the instructions laid out between the header of the loop
    that encloses the walk loop (the batch loop: reach test, rank, slot build, the next batch's gather) and the walk loop's own
    header, by kind.  A static count of the straight-line layout: every lane runs the reach test, the staged lanes the slot build."""
    body = kernel_body(asm, mangled_part)
    first = body.index(walk_loop(body)[0])
    parents = [m.group(1) for m in (re.search(r"Parent Loop (BB\d+_\d+) ", l) for l in body[first:first + 8]) if m]
    header = next(i for i, l in enumerate(body) if l.startswith(".L" + parents[-1] + ":"))
    kinds = [k for k, _ in instructions(body[header:first])]
    cnt = {c: kinds.count(c) for c in KINDS}
    return {"VALU": cnt["valu"] + cnt["v_cmp"] + cnt["trans"] + cnt["v_pk"], "v_cmp": cnt["v_cmp"], "trans": cnt["trans"],
            "SALU": cnt["salu"] + cnt["branch"], "lds": cnt["lds"], "vmem": cnt["vmem"], "wait": cnt["wait"]}


def main():
    if "--staging" in sys.argv:
        csrc = os.path.join(os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]), "autovfx_amd", "csrc") if "--tree" in sys.argv else None
        asm = assembly(csrc)
        for part in ("blend_quadrant_kernelILb0", "blend_quadrant_kernelILb1"):
            print(part, "staging per batch of 64 entries:", staging_census(asm, part))
        return
    part ="blend_quadrant_kernelILb1" if "--extra" in sys.argv else "blend_quadrant_kernelILb0"
    csrc = None
    if "--tree" in sys.argv:
        csrc = os.path.join(os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]), "autovfx_amd", "csrc")
    n, rows = stage_table(part, csrc)
    fmt = lambda v: f"{v:g}"
    print(f"{part}: {n} entr{'y' if n == 1 else 'ies'} in the loop body; counts per entry")
    if "--markdown" in sys.argv:
        print("| stage | " + " | ".join(COLS) + " |")
        print("|---|" + "---|" * len(COLS))
        for name, cnt in zip(STAGES, rows):
            print(f"| {name} | " + " | ".join(fmt(cnt[c]) for c in COLS) + " |")
        tot = {c: sum(cnt[c] for cnt in rows) for c in COLS}
        print("| **full path** | " + " | ".join(f"**{fmt(tot[c])}**" for c in COLS) + " |")
    else:
        for name, cnt in zip(STAGES, rows):
            print(f"{name:28s} " + "  ".join(f"{c}={fmt(cnt[c])}" for c in COLS))
    if "--dump" in sys.argv:
        print("\n".join(walk_loop(kernel_body(assembly(csrc), part))))


if __name__ == "__main__":
    main()
