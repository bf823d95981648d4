#!/usr/bin/env python3
"""Static instruction mix of one gfx950 kernel, per loop of its assembly listing.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -mllvm -disable-machine-licm --cuda-device-only -S -gline-tables-only \
        bio_ik_amd/csrc/bioik_hip.hip -o /tmp/k.s
    python tools/asm_loop_mix.py /tmp/k.s [_Z12k_solve_lean9SolveArgs] [rows]

Every basic block is charged to the innermost loop the assembler's comments place it in; a row is one loop: VALU instructions, then
the classes (fma / mul / add = FP64; imul = 32-bit integer multiplies, 2.4 issue slots each on gfx950; mov, cnd = v_cndmask, cmp, lane =
v_readlane / v_writelane, vint = every other VALU instruction; salu, smem, lds, wait = s_waitcnt, scratch) and the source lines
(file, line rounded to 10) most of the loop's instructions come from.  The counts are static: weigh them with the trip counts.

    python tools/asm_loop_mix.py /tmp/k.s _Z19k_solve_lean_cl64w49SolveArgs --copies [N]

lists instead every loop of the kernel that holds a run of N (default 4) or more consecutive v_mov_b32 / v_mov_b64 from a VGPR to a VGPR -- values carried
from one set of registers to another, which the `mov` class above does not tell from constants being materialised: the loop's header and depth, the block
of the run, whether that block is the loop's latch (it branches back to the header), the run's length in instructions and in dwords, and its source line.

    python tools/asm_loop_mix.py /tmp/k.s _Z19k_solve_lean_cl64w49SolveArgs --lines LO HI

lists the VALU instructions per loop and per line LO ... HI of bioik_kernels.h -- the lines of ONE phase's function, each instruction charged to the line of that
function its inlined-at chain names -- so that the instructions along the path one trip takes can be added up by hand (profiles/dense_line_search.log).
"""
import collections
import re
import sys


def classify(op):
    if op.startswith(("v_fma", "v_fmac")):
        return "fma"
    if op.startswith("v_mul_f64"):
        return "mul"
    if op.startswith("v_add_f64"):
        return "add"
    if op.startswith(("v_mov", "v_accvgpr")):
        return "mov"
    if op.startswith("v_cndmask"):
        return "cnd"
    if op.startswith("v_cmp"):
        return "cmp"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
        return "lane"
    if op.startswith(("v_mul_lo", "v_mul_hi", "v_mad_u64")):
        return "imul"
    if op.startswith("v_"):
        return "vint"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_load"):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("scratch_"):
        return "scratch"
    return "other"


VALU = ("fma", "mul", "add", "mov", "cnd", "cmp", "lane", "vint", "imul")
SHOWN = VALU + ("salu", "smem", "lds", "wait", "scratch")


VGPR_COPY = re.compile(r"^v_mov_b(32|64)(?:_e32|_e64)?\s+v(?:\d+|\[\d+:\d+\]),\s*v(?:\d+|\[\d+:\d+\])\s*(?:;.*)?$")


def copy_runs(lines, start, end, files, least):
    """runs of `least` or more consecutive VGPR-to-VGPR moves inside loops: (header, depth, block, is_latch, instructions, dwords, source)"""
    runs = []
    header, block, loc = ("top", 0), None, None
    run, dwords, run_loc = 0, 0, None
    latch = {}

    def close():
        nonlocal run, dwords
        if run >= least and header[1] > 0:
            runs.append([header[0], header[1], block, run, dwords, run_loc])
        run, dwords = 0, 0
    for i in range(start, end):
        t = lines[i]
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", t)
        if m:
            close()
            comment = m.group(2) or ""
            j = i + 1
            while j < end and lines[j].lstrip().startswith(";"):
                comment += lines[j]
                j += 1
            own = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", comment)
            inside = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", comment)
            block = m.group(1)[2:]
            header = (block, int(own.group(1))) if own else ((inside.group(1), int(inside.group(2))) if inside else ("top", 0))
            continue
        t = t.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            if int(m.group(2)):  # (line 0: compiler-made code, such as the copies at a latch; it keeps the line in front of it)
                loc = "%s:%d" % (files.get(int(m.group(1))), int(m.group(2)))
            continue
        if not t or t[0] in ";." or t.split()[0].endswith(":"):
            continue
        m = VGPR_COPY.match(t)
        if m:
            if run == 0:
                run_loc = loc
            run += 1
            dwords += 2 if m.group(1) == "64" else 1
            continue
        close()
        m = re.match(r"s_c?branch\S*\s+\.L(BB\d+_\d+)", t)
        if m and m.group(1) == header[0]:
            latch[block] = True
    close()
    return [(h, d, b, bool(latch.get(b)), n, w, src) for h, d, b, n, w, src in runs]


def line_counts(lines, start, end, lo, hi):
    """VALU instructions per (loop header, depth, line): every instruction is charged to the first bioik_kernels.h line in [lo, hi] that the inlined-at chain of its
    .loc names -- the line of the phase's own function, whatever was inlined into it (a .loc of line 0 keeps the line in front of it; code of other phases is left out)"""
    header, cur = ("top", 0), None
    count = collections.Counter()
    for i in range(start, end):
        t = lines[i]
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", t)
        if m:
            comment = m.group(2) or ""
            j = i + 1
            while j < end and lines[j].lstrip().startswith(";"):
                comment += lines[j]
                j += 1
            own = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", comment)
            inside = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", comment)
            header = (m.group(1)[2:], int(own.group(1))) if own else ((inside.group(1), int(inside.group(2))) if inside else ("top", 0))
            continue
        t = t.strip()
        if t.startswith(".loc"):
            named = [int(x) for x in re.findall(r"bioik_kernels\.h:(\d+)", t)]
            inside_range = [x for x in named if lo <= x <= hi]
            if inside_range:
                cur = inside_range[0]
            elif named and 0 not in named:
                cur = None
            continue
        if not t or t[0] in ";." or t.split()[0].endswith(":"):
            continue
        if cur is not None and classify(t.split()[0]) in VALU:
            count[(header[0], header[1], cur)] += 1
    return count


def main():
    if "--lines" in sys.argv:  # asm_loop_mix.py listing.s kernel --lines LO HI
        k = sys.argv.index("--lines")
        lo, hi = int(sys.argv[k + 1]), int(sys.argv[k + 2])
        lines = open(sys.argv[1]).read().split("\n")
        start = next(i for i, l in enumerate(lines) if l.startswith(sys.argv[2] + ":"))
        end = next(i for i, l in enumerate(lines) if i > start and l.startswith(".Lfunc_end"))
        for (h, d, line), n in sorted(line_counts(lines, start, end, lo, hi).items()):
            print("loop %-10s depth %d  bioik_kernels.h:%d  VALU %d" % (h, d, line, n))
        return
    if "--copies" in sys.argv:
        k = sys.argv.index("--copies")
        least = int(sys.argv[k + 1]) if len(sys.argv) > k + 1 else 4
        del sys.argv[k:k + 2]
    else:
        least = 0
    path = sys.argv[1]
    kernel = sys.argv[2] if len(sys.argv) > 2 else "_Z12k_solve_lean9SolveArgs"
    rows = int(sys.argv[3]) if len(sys.argv) > 3 else 25
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(kernel + ":"))
    end = next(i for i, l in enumerate(lines) if i > start and l.startswith(".Lfunc_end"))
    files = {}
    for l in lines:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            files[int(m.group(1))] = (m.group(3) or m.group(2)).split("/")[-1]
    if least:
        found = copy_runs(lines, start, end, files, least)
        print("kernel", kernel, "runs of %d or more VGPR-to-VGPR moves inside loops: %d" % (least, len(found)))
        for h, d, b, is_latch, n, w, src in sorted(found, key=lambda r: (-r[1], -r[4])):
            print("depth %d  loop %-10s block %-10s %-5s %2d moves %2d dwords  %s" % (d, h, b, "latch" if is_latch else "body", n, w, src))
        return
    header, loc = ("top", 0), None
    count = collections.defaultdict(collections.Counter)
    source = collections.defaultdict(collections.Counter)
    for i in range(start, end):
        t = lines[i]
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", t)
        if m:
            comment = m.group(2) or ""
            j = i + 1
            while j < end and lines[j].lstrip().startswith(";"):
                comment += lines[j]
                j += 1
            own = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", comment)
            inside = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", comment)
            header = (m.group(1)[2:], int(own.group(1))) if own else ((inside.group(1), int(inside.group(2))) if inside else ("top", 0))
            continue
        t = t.strip()
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            loc = (files.get(int(m.group(1))), int(m.group(2)) // 10 * 10)
            continue
        if not t or t[0] in ";." or t.split()[0].endswith(":"):
            continue
        count[header][classify(t.split()[0])] += 1
        if loc:
            source[header][loc] += 1
    total = collections.Counter()
    for c in count.values():
        total += c
    print("kernel", kernel, {k: total[k] for k in SHOWN if total[k]})
    ranked = sorted(count.items(), key=lambda kv: -sum(kv[1][x] for x in VALU))
    for h, c in ranked[:rows]:
        print(sum(c[x] for x in VALU), h, {k: c[k] for k in SHOWN if c[k]}, source[h].most_common(3))


if __name__ == "__main__":
    main()
