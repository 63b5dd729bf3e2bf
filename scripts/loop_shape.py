#!/usr/bin/env python3
"""Shape of the band kernels' plain (non-check) iteration: for every pdhg_band_kernel instantiation, and for each wave
kind (wave 0 with the tau column's reduction, marked by its s_setprio; the other waves), whether the plain iteration is
an innermost loop holding both of the iteration's barriers, and what it issues: VALU instructions, FP64 arithmetic
among them (v_fma / v_fmac / v_add / v_mul _f64, what the FMA / ADD / MUL counters of scripts/pmc_valu.py count),
register-to-register v_mov_b64, branches, scratch loads / stores (gfx950 ISA from hipcc -S with the library's per-source
flags, as scripts/spill_sites.py).  It reports only.

An iteration body is a set of blocks with exactly two barriers, the read of the iteration's Halpern weight (v_readlane)
and at least the FP64 work of one update of the lane's columns and rows.  Of a wave kind's bodies the plain one is the
shorter (the check iteration also stores the images and sums the movements).  Where the body is a loop whose child loops
hold no barrier, its blocks are counted, the rarely taken ones (the Halpern weights' reload every 64 iterations) and the
back edge included, and the kind of branch that leaves it is printed (s_cbranch_scc*: a scalar exit).  Where it is not
(the body is part of a larger region, entered and left through a chain of flag-driven branches) the layout span from the
branch target that opens it to its second barrier is counted, and the longest run of register-to-register v_mov_b64
among the region's other blocks is printed beside it: the copies of the new iterate back to the registers the next
iteration reads, executed once per iteration.

Usage: python scripts/loop_shape.py [file.hip ...]   (default: the band units)
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from spill_sites import isa  # noqa: E402
from spills import short  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "der-vet_amd", "csrc")
DEFAULT = ["dvh_band_persist.hip", "dvh_band_persist_ice.hip", "dvh_band.hip"]
FP64 = re.compile(r"^v_(fma|fmac|add|mul)_f64")  # (as the FMA / ADD / MUL counters of scripts/pmc_valu.py)
MOV64 = re.compile(r"^v_mov_b64(_e32|_e64)?\s+v\[\d+:\d+\],\s*v\[\d+:\d+\]\s*$")


class Block:
    def __init__(self, label, note):
        self.label, self.note, self.ins = label, note, []
        m = re.search(r"Loop Header: Depth=(\d+)", note) or re.search(r"in Loop: Header=\S+ Depth=(\d+)", note)
        self.depth = int(m.group(1)) if m else 0
        self.header = "Loop Header" in note
        m = re.findall(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", note)
        self.parent = next((".L" + lab for lab, d in m if int(d) == self.depth - 1), None) if self.header else None
        m = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
        self.loop = "." + "L" + m.group(1) if m else (label if self.header else None)


def blocks_of(body):
    out, cur = [], Block("entry", "")
    for k, ln in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+|; %bb\.\d+):(.*)$", ln)
        if m:
            note = m.group(2)
            # a loop header's annotation continues on the comment lines that follow the label
            j = k + 1
            while j < len(body) and body[j].startswith("      ") and ";" in body[j][:60] and not body[j].startswith("\t"):
                note += " " + body[j].strip()
                j += 1
            out.append(cur)
            cur = Block(m.group(1), note)
            continue
        t = ln.strip()
        if ln.startswith("\t") and t and not t.startswith((".", ";")):
            cur.ins.append(t.split(";")[0].strip())
    out.append(cur)
    return out


def count(ins):
    valu = [i for i in ins if i.startswith("v_")]
    return {"valu": len(valu), "fp64": sum(1 for i in valu if FP64.match(i)),
            "mov64": sum(1 for i in valu if MOV64.match(i)),
            "branch": sum(1 for i in ins if i.startswith(("s_cbranch", "s_branch"))),
            "scratch": sum(1 for i in ins if i.startswith("scratch_")),
            "barriers": sum(1 for i in ins if i.startswith("s_barrier"))}


def mov_run(blocks):
    best = 0
    for b in blocks:
        run = 0
        for i in b.ins:
            run = run + 1 if MOV64.match(i) else 0
            best = max(best, run)
    return best


def bodies(blocks, min_fp64):
    """Iteration bodies: sets of blocks that hold exactly two barriers, at least min_fp64 FP64 instructions (an
    iteration updates every column and row of the lane's steps; the check path's barrier pairs hold less) and the read
    of the iteration's Halpern weight."""
    found = []
    own, kids = {}, {}
    for k, b in enumerate(blocks):
        if b.loop:
            own.setdefault(b.loop, []).append(k)
        if b.header and b.parent:
            kids.setdefault(b.parent, []).append(b.label)

    def members(lab):
        return own.get(lab, []) + [k for c in kids.get(lab, []) for k in members(c)]

    def nbar(ks):
        return sum(1 for k in ks for i in blocks[k].ins if i.startswith("s_barrier"))

    def add(ks, loop, nkids):
        ins = [i for q in ks for i in blocks[q].ins]
        # (the Halpern weight of the iteration comes through v_readlane; the power iteration's loop has none)
        if count(ins)["fp64"] >= min_fp64 and any(i.startswith("v_readlane_b32") for i in ins):
            found.append({"blocks": ks, "loop": loop, "kids": nkids, "w0": any(i.startswith("s_setprio 2") for i in ins)})
            return True
        return False

    taken = set()
    # loops with both barriers of an iteration and none in a child loop
    for lab in own:
        ks = sorted(members(lab))
        if nbar(ks) == 2 and all(nbar(members(c)) == 0 for c in kids.get(lab, [])) and add(ks, True, len(kids.get(lab, []))):
            taken.update(ks)
    # bodies that are part of a larger region: the layout span from the branch target that opens the body (a block
    # the one before it does not fall into) over conditional skips and child loops to the second barrier
    k = 0
    while k < len(blocks):
        if k in taken or nbar([k]) == 0:
            k += 1
            continue
        j, nb = k, 0
        while j < len(blocks) and j not in taken:
            nb += nbar([j])
            if nb >= 2 or (blocks[j].ins and blocks[j].ins[-1].startswith(("s_branch", "s_endpgm"))):
                break
            j += 1
        if nb == 2 and j < len(blocks):
            i0 = k
            while i0 > 0 and i0 - 1 not in taken and nbar([i0 - 1]) == 0 and \
                    not (blocks[i0 - 1].ins and blocks[i0 - 1].ins[-1].startswith("s_branch")):
                i0 -= 1
            add(list(range(i0, j + 1)), False, 0)
            k = j + 1
        else:
            k += 1
    return found


def report(path):
    lines = isa(path)
    fns = [(i, re.search(r"\.type\s+(\S+),@function", ln).group(1)) for i, ln in enumerate(lines) if "@function" in ln]
    for n, (s0, name) in enumerate(fns):
        if "pdhg_band_kernel" not in name:
            continue
        blocks = blocks_of(lines[s0:fns[n + 1][0] if n + 1 < len(fns) else len(lines)])
        targs = [int(v) for v in re.findall(r"\d+", short(name).split("<", 1)[-1])]  # B, S, ICE, ...
        steps, ice = targs[1], targs[2]
        found = bodies(blocks, 3 * steps * (9 if ice else 5))
        print(f"{os.path.basename(path)}  {short(name)}")
        for w0 in (True, False):
            who = "wave 0     " if w0 else "other waves"
            cand = [f for f in found if f["w0"] == w0]
            if not cand:
                print(f"    {who}: no iteration body found")
                continue
            # the plain iteration: the body with the fewest VALU instructions
            f = min(cand, key=lambda f: count([i for q in f["blocks"] for i in blocks[q].ins])["valu"])
            c = count([i for q in f["blocks"] for i in blocks[q].ins])
            first = blocks[f["blocks"][0]]
            tail = ""
            if f["loop"]:
                # the branches that leave the loop (scalar: s_cbranch_scc*)
                inside = {blocks[q].label for q in f["blocks"]}
                exits = sorted({i.split()[0] for q in f["blocks"] for i in blocks[q].ins
                                if i.startswith("s_cbranch") and i.split()[1] not in inside})
                tail = "  exit: " + ", ".join(exits)
                shape = "innermost loop, both barriers inside" if f["kids"] == 0 else \
                    f"loop of its own, both barriers inside, innermost but for {f['kids']} barrier-free loops over the tau columns"
            else:
                shape = "NOT a loop of its own"
                region = [b for q, b in enumerate(blocks) if q not in f["blocks"] and b.depth == first.depth]
                tail = f"  (+ a run of {mov_run(region)} v_mov_b64 reg-reg elsewhere in the depth-{first.depth} region)"
            print(f"    {who}: {shape} ({first.label} .. {blocks[f['blocks'][-1]].label}, depth {first.depth}): "
                  f"VALU {c['valu']}, FP64 arithmetic {c['fp64']}, v_mov_b64 reg-reg {c['mov64']}, "
                  f"branches {c['branch']}, scratch {c['scratch']}{tail}")


def main(argv):
    for f in argv or DEFAULT:
        report(f if os.path.exists(f) else os.path.join(CSRC, f))


if __name__ == "__main__":
    main(sys.argv[1:])
