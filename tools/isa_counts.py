"""Dev: static instruction counts of one kernel, per basic block, from gfx950 assembly.

    python tools/isa_counts.py csrc/gram_solve.hip 'gram_solve_kernel<4, false>'
    python tools/isa_counts.py build/gram_solve.s  'gram_solve_kernel<4, false>' --hist 12

A `.hip` source is compiled to device assembly first (the Makefile's flags); a `.s` file is
read as it is.  The kernel is chosen by a substring of its demangled name (exactly one kernel
must match).  Per basic block: VALU (every `v_` instruction but the matrix-core ones), MFMA,
LDS (`ds_`), VMEM (`global_` / `buffer_` / `flat_` / `scratch_`), SMEM (`s_load` /
`s_buffer_load`), SALU (the other `s_`, without `s_nop` / `s_waitcnt`), and whether the block
lies in a loop (a cycle of the control-flow graph).  The loops that
issue f16 matrix-core products are the Gram loop(s); everything else of a row (prologue,
guards, regularisation, the unrolled block elimination, the store) is "outside the Gram
loop", the figure tests/test_gram_solve_valu_cpu.py holds the rank-64 kernel to.
`--hist N` adds the N most frequent VALU mnemonics outside the Gram loop.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recommender-system-using-apache-spark-mllib-_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KINDS = ("valu", "mfma", "lds", "vmem", "smem", "salu")
_LABEL = re.compile(r"^([_A-Za-z.$][\w.$]*):")


def compile_to_asm(src: str, out: str) -> None:
    """Device assembly of a HIP source at the library's flags."""
    p = subprocess.run([HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-I", CSRC,
                        "--offload-device-only", "-S", src, "-o", out],
                       capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError(p.stderr[-3000:])


def kind_of(op: str):
    if op.startswith(("v_mfma", "v_smfmac")):
        return "mfma"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith("s_") and not op.startswith(("s_nop", "s_waitcnt")):
        return "salu"
    return None


def _demangle(names):
    p = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, p.stdout.split("\n")))


def kernel_names(lines):
    """Mangled names of the kernels a device assembly file defines."""
    return [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m]


def find_kernel(lines, name_filter: str) -> str:
    dm = _demangle(kernel_names(lines))
    want = name_filter.replace(" ", "")
    hits = [k for k, v in dm.items() if want in v.replace(" ", "")]
    if len(hits) != 1:
        raise KeyError(f"{name_filter!r} matches {len(hits)} kernels: "
                       + ", ".join(dm[h][:80] for h in hits[:6]))
    return hits[0]


def blocks_of(lines, mangled: str):
    """[{label, ops: [mnemonic], targets: [label]}] of one function, in layout order."""
    blocks, cur, inside = [], None, False
    for raw in lines:
        line = raw.split(";")[0].rstrip()
        if not line.strip():
            continue
        m = _LABEL.match(line)
        if m:
            lab = m.group(1)
            if lab == mangled:
                inside = True
            elif inside and (lab.startswith(".Lfunc_end") or not lab.startswith(".L")):
                break
            if inside:
                cur = {"label": lab, "ops": [], "targets": []}
                blocks.append(cur)
            continue
        ins = line.strip()
        if not inside or ins.startswith("."):
            continue
        parts = ins.replace(",", " ").split()
        cur["ops"].append(parts[0])
        if parts[0].startswith(("s_cbranch", "s_branch")) and len(parts) > 1:
            cur["targets"].append(parts[1])
    return blocks


def loop_sets(blocks):
    """The loops of a function as sets of block numbers: the strongly connected components
    of its control-flow graph that hold an edge (branch targets, and the fall-through
    unless the block ends in s_branch / s_endpgm / s_setpc)."""
    index = {b["label"]: i for i, b in enumerate(blocks)}
    succ = []
    for n, b in enumerate(blocks):
        out = {index[t] for t in b["targets"] if t in index}
        last = b["ops"][-1] if b["ops"] else ""
        if n + 1 < len(blocks) and not last.startswith(("s_branch", "s_endpgm", "s_setpc")):
            out.add(n + 1)
        succ.append(out)

    def reach(n):
        seen, todo = set(), list(succ[n])
        while todo:
            x = todo.pop()
            if x not in seen:
                seen.add(x)
                todo.extend(succ[x])
        return seen

    fwd = [reach(n) for n in range(len(blocks))]
    sets = []
    for n in range(len(blocks)):
        if n in fwd[n] and not any(n in s for s in sets):
            sets.append({x for x in fwd[n] if n in fwd[x]})
    return sets


def count(lines, name_filter: str) -> dict:
    """Per-block and total counts of the kernel whose demangled name holds `name_filter`."""
    mangled = find_kernel(lines, name_filter)
    blocks = blocks_of(lines, mangled)
    loops = loop_sets(blocks)
    gram = [scc for scc in loops
            if any(op.startswith("v_mfma") and op.endswith("f16")
                   for n in scc for op in blocks[n]["ops"])]
    rows = []
    hist = collections.Counter()
    total = dict.fromkeys(KINDS, 0)
    outside = dict.fromkeys(KINDS, 0)
    for n, b in enumerate(blocks):
        c = dict.fromkeys(KINDS, 0)
        for op in b["ops"]:
            kd = kind_of(op)
            if kd:
                c[kd] += 1
        in_loop = any(n in scc for scc in loops)
        in_gram = any(n in scc for scc in gram)
        for kd in KINDS:
            total[kd] += c[kd]
            if not in_gram:
                outside[kd] += c[kd]
        if not in_gram:
            hist.update(op for op in b["ops"] if kind_of(op) == "valu")
        rows.append(dict(c, label=b["label"], loop=in_loop, gram=in_gram))
    return {"kernel": _demangle([mangled])[mangled], "blocks": rows, "total": total,
            "outside_gram_loop": outside, "valu_hist_outside": hist}


def count_source(path: str, name_filter: str) -> dict:
    """count() of a `.s` file, or of a `.hip` source compiled first."""
    if path.endswith(".s"):
        with open(path) as f:
            return count(f.read().split("\n"), name_filter)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "kernel.s")
        compile_to_asm(path, out)
        with open(out) as f:
            return count(f.read().split("\n"), name_filter)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("source", help=".hip source or .s device assembly")
    ap.add_argument("kernel", help="substring of the kernel's demangled name")
    ap.add_argument("--hist", type=int, default=0, metavar="N",
                    help="the N most frequent VALU mnemonics outside the Gram loop")
    ap.add_argument("--min", type=int, default=1, metavar="N",
                    help="list only blocks of at least N counted instructions")
    args = ap.parse_args()
    r = count_source(args.source, args.kernel)
    print(r["kernel"][:100])
    print(f"{'block':40s} {'where':6s}" + "".join(f"{k.upper():>7s}" for k in KINDS))
    for b in r["blocks"]:
        if sum(b[k] for k in KINDS) < args.min:
            continue
        where = "gram" if b["gram"] else ("loop" if b["loop"] else "")
        print(f"{b['label'][:40]:40s} {where:6s}" + "".join(f"{b[k]:7d}" for k in KINDS))
    for title, key in (("total", "total"), ("outside the Gram loop", "outside_gram_loop")):
        print(f"{title:47s}" + "".join(f"{r[key][k]:7d}" for k in KINDS))
    if args.hist:
        for op, n in r["valu_hist_outside"].most_common(args.hist):
            print(f"  {n:5d}  {op}")


if __name__ == "__main__":
    sys.exit(main())
