"""VALU instructions of a kernel's sample loop by gfx950 issue class and by region (development tool).

Reads the listing of ONE kernel (label ... s_endpgm, as tools/isa_mix.py kernel_lines cuts it out of `make asm` output)
and uses the loop comments the compiler writes next to every block label: the sample loop is the first loop of depth 2,
blocks of depth 3 inside it are the rejection loops (tails).  Regions are cut at the s_barrier instructions and at the
first v_mbcnt of the two park steps, which is enough to tell the phases of render_kernel_coop2 apart.
usage: python tools/isa_loop.py kernel.s"""
import collections
import re
import sys

from isa_mix import classify


def blocks(lines):
    """[(label, header, depth, [instructions])]: basic blocks with the loop the compiler's comments put them in."""
    out, cur, comment = [], None, []
    for line in lines:
        m = re.match(r"(\.LBB\d+_\d+):|; %bb\.(\d+):", line)
        if m or (cur is not None and re.match(r"\s+;\s+(Parent Loop|=>|in Loop|Child Loop)", line) and not cur[3]):
            if m:
                cur = [m.group(1) or "bb" + m.group(2), None, 0, []]
                out.append(cur)
            for h, d in re.findall(r"(?:Header=|Loop )(BB\d+_\d+) Depth=(\d+)", line):
                if int(d) == 2:
                    cur[1] = h
                cur[2] = max(cur[2], int(d))
            d = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", line)
            if d:
                cur[2] = max(cur[2], int(d.group(1)))
                if int(d.group(1)) == 2:
                    cur[1] = cur[0].replace(".L", "")
            continue
        ins = re.match(r"\s+([vs]_[a-z0-9_]+|ds_[a-z0-9_]+|global_[a-z0-9_]+)\b", line)
        if ins and cur is not None:
            cur[3].append(ins.group(1))
    return out


def main():
    bl = blocks(open(sys.argv[1]).read().splitlines())
    loop = next(b[1] for b in bl if b[2] == 2 and b[1])
    body = [b for b in bl if b[1] == loop]
    for name, pick in (("sample loop, depth 2 (dense)", lambda b: b[2] == 2), ("rejection loops, depth 3", lambda b: b[2] == 3)):
        counts, lanes = collections.Counter(), collections.Counter()
        for b in body:
            if pick(b):
                for op in b[3]:
                    if op.startswith("v_"):
                        counts[classify(op)] += 1
                        if "lane_b32" in op and "first" not in op:
                            lanes[op] += 1
        print(f"{name}: VALU {sum(counts.values())}", dict(counts), "spill moves", dict(lanes))


if __name__ == "__main__":
    main()
