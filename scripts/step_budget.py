#!/usr/bin/env python3
"""Where a march step's VALU issue time goes, from a `hipcc -S` listing of the product build.

For every march loop of k_trace<0,false,false> (primary unit step, long-ray step, primary segment
step, post-drain segment step, fused prepass step) and the prepass loop of k_camerarays_group it
prints the VALU instructions and the modelled issue cycles ON THE TAKEN PATH, by category:

  octave body | steep noise | octave count + fast-cell test | density pow | terraces and floor lift |
  step pow | march update and liveness | register copies (v_mov* of a register) | lane moves

Costs are the measured ones of profiles/r02/ubench_cost_model.md: 2.4 cycles for full-rate FP32 /
integer / compare / move, 4.3 for packed FP32, conversions, floor, perm, shifts, 3-operand integer
and 64-bit ops, 8 for transcendentals.  The octave body is one iteration of the FAST FBM loop (or,
in a segment loop, the unrolled rounds); --octaves weights it for the per-step total.

The taken path: the octave-count estimate is accepted (no exact fallback), the cells take the
short integer path (FAST), no pow argument is out of range, and the terraces, the floor lift and
both march branches (hit / step) run; a finished ray's results and a lane refill, which sit
inside the long-ray and segment loops but run per ray, are left out.  Blocks off that path are recognised by what they hold
(v_sqrt_f32: the exact octave count; a texel offset from v_cvt_i32_f32 and a shift by 9: the
general cell path; a short block with a v_med3_f32: the clamp of a pow's rare lanes); a loop's inner FBM loops are octave bodies.
Loops are told apart by structure: see classify().  Categories follow the literals of the source
(-0.2: end of the steep noise, 5.0: the step factor's base) in layout order, so an instruction the
scheduler moved across a boundary counts with its neighbours.  In a segment march the steep noise is
one of the unrolled octave rounds; its "steep noise" and "terraces and floor lift" rows are one term
(whichever side of the -0.2 the compiler put the code on).

  python3 scripts/step_budget.py [--listing k.s] [--octaves 11.1]
Without --listing the tree's rt_kernels.hip is compiled with the flags of csrc/Makefile."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CSRC = os.path.join(ROOT, "gpgpuraytrace_amd", "csrc")
K_TRACE = "_ZN12_GLOBAL__N_17k_traceILi0ELb0ELb0EE"
K_PREPASS = "_ZN12_GLOBAL__N_118k_camerarays_groupILb0ELi512ELi8EE"

FULL = re.compile(r"v_(add|sub|subrev|mul|fma|fmac|fmamk|fmaak|max|min)_f32|v_(and|or|xor|add|sub|subrev)_(b32|u32|co_u32)|"
                  r"v_subb?rev_co_u32|v_cmp|v_mov_b32|v_cndmask")
TRANS = re.compile(r"v_(exp|log|rcp|rsq|sqrt|sin|cos)_f32")
CATS = ["octave body", "steep noise", "octave count + fast-cell test", "density pow", "terraces and floor lift",
        "step pow", "march update and liveness", "register copies", "lane moves"]


def cost(op):
    if TRANS.match(op):
        return 8.0
    if FULL.match(op) and not op.startswith("v_pk"):
        return 2.4
    return 4.3


def listing_of_tree():
    out = os.path.join(tempfile.mkdtemp(prefix="step_budget_"), "k.s")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "--cuda-device-only", "-S", "rt_kernels.hip", "-o", out]
    subprocess.run(cmd, cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
    return out


def blocks_of(lines, prefix):
    """The kernel's basic blocks in layout order: name, loop (innermost header), instruction lines."""
    start = next(i for i, l in enumerate(lines) if l.startswith(prefix) and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur, parent = [], None, {}
    for l in lines[start:end]:
        m = re.match(r"^(\.LBB\w+|; %bb\.\d+):(.*)$", l)
        if m:
            cur = {"name": m.group(1), "ann": m.group(2), "ins": []}
            blocks.append(cur)
            continue
        if cur is None:
            continue
        st = l.strip()
        if st.startswith(";") and "Loop" in st:
            cur["ann"] += " " + st
        elif l.startswith("\t") and st and not st.startswith((".", ";")):
            cur["ins"].append(st)
    for b in blocks:
        a = b["ann"]
        if "Loop Header" in a:
            b["loop"] = b["name"].replace(".LBB", "")
            ps = re.findall(r"Parent Loop BB(\d+_\d+)", a)
            parent[b["loop"]] = ps[-1] if ps else None
        else:
            m = re.search(r"in Loop: Header=BB(\d+_\d+)", a)
            b["loop"] = m.group(1) if m else None
    return blocks, parent


def is_body(b):
    return sum(1 for i in b["ins"] if i.startswith("ds_read_b128")) >= 4


def general_cells(b):
    return any(re.match(r"v_lshlrev_b32_e32 v\d+, 9,", i) for i in b["ins"]) and any(i.startswith("v_cvt_i32_f32") for i in b["ins"])


def classify(blocks, parent):
    """march loops -> name.  A lane-per-ray march holds its FBM as one pair of inner loops (FAST and
    general); the primary unit step is the one that raises the wave priority (s_setprio), the long-ray
    step the other.  A segment march holds the octave bodies unrolled in its own blocks: the primary
    segment step is nested in the primary unit's frame loop, and of the other two the one with more
    blocks (it finishes rays: long_finish) is the post-drain segment step, the other the fused prepass."""
    own = collections.defaultdict(list)
    for b in blocks:
        if b["loop"]:
            own[b["loop"]].append(b)
    kids = collections.defaultdict(list)
    for l, p in parent.items():
        if p:
            kids[p].append(l)
    body_loop = {l for l, bs in own.items() if len(bs) == 1 and is_body(bs[0])}
    names = {}
    lane = [l for l in own if len([k for k in kids[l] if k in body_loop]) == 2]
    for l in lane:
        prio = any(i.startswith("s_setprio") for b in own[l] for i in b["ins"])
        names[l] = "primary unit step" if prio else "long-ray step"
    seg = [l for l in own if l not in body_loop and any(is_body(b) for b in own[l]) and
           any(i.startswith("v_frexp_mant") for b in own[l] for i in b["ins"]) and not kids[l]]
    prim_parent = {parent[l] for l, n in names.items() if n == "primary unit step"}
    rest = []
    for l in seg:
        if parent.get(l) in prim_parent:
            names[l] = "primary segment step"
        else:
            rest.append(l)
    rest.sort(key=lambda l: -len(own[l]))
    for l, n in zip(rest, ["post-drain segment step", "fused prepass step"]):
        names[l] = n
    return names, own, kids, body_loop


def taken_stream(loop, blocks, own, kids, body_loop):
    """(category override or None, instruction) along the taken path of the loop, in layout order."""
    inner = set(kids[loop])
    span = [b for b in blocks if b["loop"] == loop or b["loop"] in inner]
    # the step: the liveness test at the loop's head (the blocks before its first memory or queue
    # operation), then everything from the block that starts the density sample (the octave count's
    # v_log_f32) on.  What lies between (a finished ray's results, a refill from the ring) runs per
    # ray, not per step.
    first = next(n for n, b in enumerate(span) if any(i.startswith("v_log_f32") for i in b["ins"]))
    rare = ("global_", "flat_", "buffer_", "ds_", "s_sleep", "s_barrier")
    head = next((n for n, b in enumerate(span[:first]) if any(i.startswith(rare) for i in b["ins"])), first)
    span = span[:head] + span[first:]
    out, skip_to = [], None
    for n, b in enumerate(span):
        if skip_to:
            if b["name"] != skip_to:
                continue
            skip_to = None
        if b["loop"] in inner:
            if b["loop"] in body_loop and not any(i.startswith("v_cvt_i32_f32") for i in b["ins"]):
                out += [("octave body", i) for i in b["ins"]]  # the FAST FBM loop; the general one is off the path
            continue
        ins = b["ins"]
        if any(i.startswith("v_sqrt_f32") for i in ins):  # (a fallback reached without a guard block: never taken)
            continue
        if general_cells(b) and not is_body(b):
            continue
        if len(ins) < 8 and any(i.startswith("v_med3_f32") for i in ins):
            continue  # a wave-tested pow's clamp block (v_med3_f32 with -150 and 128, and the rounding again)
        out += [("octave body" if is_body(b) else None, i) for i in ins]
        # the exact octave count: guarded by s_cbranch_execz over blocks the next of which holds v_sqrt_f32
        m = re.match(r"s_cbranch_execz (\S+)", ins[-1]) if ins else None
        if m and n + 1 < len(span) and any(i.startswith("v_sqrt_f32") for i in span[n + 1]["ins"]):
            skip_to = m.group(1)
    return out


def budget(stream, lane, show=None):
    cat, seen_body = "march update and liveness", False
    count, cyc = collections.Counter(), collections.Counter()
    for forced, i in stream:
        op = i.split()[0]
        if forced:
            seen_body = True
            if lane:
                cat = "density pow"  # what follows the FBM loop
        elif op.startswith("v_log_f32") and not seen_body:
            cat = "octave count + fast-cell test"
        elif seen_body and cat == "octave count + fast-cell test":
            # a segment march's gathers and weighted sum count with its octave rounds, up to the density pow
            cat = "density pow" if op.startswith("v_frexp") else cat
        elif "0xbe4ccccd" in i:
            cat = "terraces and floor lift"
        elif "0x40a00000" in i:
            cat = "step pow"
        if not op.startswith("v_"):
            continue
        c = forced or ("octave body" if seen_body and cat == "octave count + fast-cell test" else cat)
        if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
            c = "lane moves"
        elif re.match(r"v_mov_b\d+_e\d+ v\S+ v", i.replace(",", "")) and "row_" not in i and "quad_perm" not in i:
            c = "register copies"
        count[c] += 1
        cyc[c] += cost(op)
        if show == c:
            print("    " + i)
        if not forced and op.startswith("v_ldexp"):
            if cat == "density pow":
                cat = "steep noise"
            elif cat == "step pow":
                cat = "march update and liveness"
    return count, cyc


def report(path, prefix, title, octaves, show):
    lines = open(path).read().split("\n")
    blocks, parent = blocks_of(lines, prefix)
    names, own, kids, body_loop = classify(blocks, parent)
    if prefix == K_PREPASS:
        names = {l: "prepass step" for l, n in names.items() if "segment" in n or "prepass" in n}
    print(f"\n### {title}\n")
    for loop in sorted(names, key=lambda l: names[l]):
        lane = names[loop] in ("primary unit step", "long-ray step")
        if show:
            print(f"{names[loop]}: {show}")
        count, cyc = budget(taken_stream(loop, blocks, own, kids, body_loop), lane, show)
        w = octaves if lane else 1.0
        total = sum(cyc[c] * (w if c == "octave body" else 1.0) for c in CATS)
        print(f"**{names[loop]}** (loop BB{loop}" + (f", octave body x {octaves}" if lane else ", octave rounds unrolled") + ")\n")
        print("| category | VALU | issue cycles | share of a step |")
        print("|---|---:|---:|---:|")
        for c in CATS:
            cy = cyc[c] * (w if c == "octave body" else 1.0)
            print(f"| {c} | {count[c]} | {cyc[c]:.0f}" + (f" x {w} = {cy:.0f}" if lane and c == "octave body" else "") +
                  f" | {100 * cy / total:.1f}% |")
        rest = sum(count[c] for c in CATS if c != "octave body")
        print(f"| **non-octave** | {rest} | {total - cyc['octave body'] * w:.0f} | {100 * (1 - cyc['octave body'] * w / total):.1f}% |")
        print(f"| **step** | | {total:.0f} | |\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--listing", help="a hipcc -S listing of rt_kernels.hip (default: compile the tree's)")
    ap.add_argument("--octaves", type=float, default=11.1, help="octaves per density sample that weight the octave body")
    ap.add_argument("--show", metavar="CATEGORY", help="also list each loop's instructions of this category")
    a = ap.parse_args()
    path = a.listing or listing_of_tree()
    report(path, K_TRACE, "k_trace<0, false, false>", a.octaves, a.show)
    report(path, K_PREPASS, "k_camerarays_group<false, 512, 8>", a.octaves, a.show)


if __name__ == "__main__":
    sys.exit(main())
