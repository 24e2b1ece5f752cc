#!/usr/bin/env python3
"""Per-kernel diff of two `make asm` outputs (a refactor's proof of no change).

  python tools/isa_diff.py OLD.s NEW.s [--diff]

Pairs the functions of the two files by name (RENAMED maps the names a
refactor changed), strips comments and directives, renumbers the local labels
in order of appearance and replaces function symbols by their paired names,
then prints for each kernel "identical" or the number of differing lines with
the old -> new vgpr_count, sgpr_count, vgpr_spill_count, sgpr_spill_count,
private_segment_fixed_size and instruction count.  Device functions that are
real calls (the __noinline__ cold paths) are compared the same way, without
the metadata; --diff adds the unified diff of every pair that differs.  A
plain diff: it looks for no particular instruction.  Exit status 1 when any
pair differs or a function has no partner."""
import difflib
import re
import sys

# old symbol -> new symbol, for kernels a change renamed on purpose
RENAMED = {
    # one scatter template for the binned and the dense path
    "_ZN2sa12_GLOBAL__N_118bt_scatter2_kernelILi0EEEvNS_12IngestParamsE":
        "_ZN2sa12_GLOBAL__N_118bt_scatter2_kernelINS0_8BtHashedELi0EEEvNS_12IngestParamsE",
    "_ZN2sa12_GLOBAL__N_117dn_scatter_kernelENS_12IngestParamsE":
        "_ZN2sa12_GLOBAL__N_118bt_scatter2_kernelINS0_7BtDenseELi0EEEvNS_12IngestParamsE",
    # ingest kernels without their retired template parameters
    "_ZN2sa12_GLOBAL__N_117ingest_lds_kernelILi0ELi4ELb1ELb0ELi0EEEvNS_12IngestParamsE":
        "_ZN2sa12_GLOBAL__N_117ingest_lds_kernelENS_12IngestParamsE",
    "_ZN2sa12_GLOBAL__N_117ingest_hbm_kernelILi16ELi4ELb0ELi256EEEvNS_12IngestParamsE":
        "_ZN2sa12_GLOBAL__N_117ingest_hbm_kernelILi16EEEvNS_12IngestParamsE",
    "_ZN2sa12_GLOBAL__N_117ingest_hbm_kernelILin1ELi4ELb0ELi256EEEvNS_12IngestParamsE":
        "_ZN2sa12_GLOBAL__N_117ingest_hbm_kernelILin1EEEvNS_12IngestParamsE",
    "_ZN2sa12_GLOBAL__N_119part_scatter_kernelILi16ELb1EEEvNS_12IngestParamsE":
        "_ZN2sa12_GLOBAL__N_119part_scatter_kernelILi16EEEvNS_12IngestParamsE",
    "_ZN2sa12_GLOBAL__N_119part_scatter_kernelILin1ELb1EEEvNS_12IngestParamsE":
        "_ZN2sa12_GLOBAL__N_119part_scatter_kernelILin1EEEvNS_12IngestParamsE",
    # (the laboratory build's small-table ablation instance: LabV2<...> -> V2Diag)
    "_ZN2sa12_GLOBAL__N_116ingest_v2_kernelILi0ELi0ELi0ELb0ELj1024ENS0_5LabV2ILi2ELi2ELi2ELb1ELin1ELb1ELi0ELb0ELb0ELb0ELb0EEEEEvNS_12IngestParamsE":
        "_ZN2sa12_GLOBAL__N_116ingest_v2_kernelILi0ELi0ELi0ELb0ELj1024ENS0_6V2DiagEEEvNS_12IngestParamsE",
    # (the laboratory build now takes the 512-thread kernel from the product's option set: LabV2<...> -> V2Lean)
    "_ZN2sa12_GLOBAL__N_116ingest_v2_kernelILi0ELi0ELi0ELb0ELj512ENS0_5LabV2ILi2ELi2ELi2ELb0ELin1ELb1ELi1ELb1ELb1ELb0ELb0EEEEEvNS_12IngestParamsE":
        "_ZN2sa12_GLOBAL__N_116ingest_v2_kernelILi0ELi0ELi0ELb0ELj512ENS0_6V2LeanEEEvNS_12IngestParamsE",
    # the latency range sums, named for what they sum: n_ranges in {1, 2}
    "_ZN2sa12_GLOBAL__N_120lat_pair_sums_kernelEPKyjjmjmjjjjPy":
        "_ZN2sa12_GLOBAL__N_121lat_range_sums_kernelEPKyjjmjmjjjjPy",
}
# (the laboratory build's ablation instances: <MODE> -> <BtHashed, MODE>)
for _m in (1, 2, 3, 4, 8, 16, 32, 64):
    RENAMED[f"_ZN2sa12_GLOBAL__N_118bt_scatter2_kernelILi{_m}EEEvNS_12IngestParamsE"] = \
        f"_ZN2sa12_GLOBAL__N_118bt_scatter2_kernelINS0_8BtHashedELi{_m}EEEvNS_12IngestParamsE"

META = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
SYMBOL = re.compile(r"\b_Z\w+")
LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?\b")


def parse(path, rename):
    """{name: (normalised lines, instruction count)}, {kernel name: metadata}"""
    lines = open(path).read().splitlines()
    funcs, meta = {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.type\s+(\S+),@function", lines[i])
        if not m:
            i += 1
            continue
        name = rename.get(m.group(1), m.group(1))
        body, labels, n_ins = [], {}, 0
        i += 2  # the .type line and the function's own label
        while i < len(lines) and not re.match(r"\.Lfunc_end\d+:", lines[i]):
            t = lines[i].split(";")[0].strip()
            i += 1
            if not t or (t.startswith(".") and not t.endswith(":")):
                continue  # comment, blank or directive (the kernel descriptor block among them)
            t = SYMBOL.sub(lambda s: rename.get(s.group(0), s.group(0)), t)
            t = LABEL.sub(lambda s: labels.setdefault(s.group(0), f".L{len(labels)}"), t)
            n_ins += 0 if t.endswith(":") else 1
            body.append(t)
        funcs[name] = (body, n_ins)
    cur = {}
    for l in lines:
        if re.match(r"  - \.", l):  # a new kernel's entry of amdhsa.kernels
            cur = {}
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)\s*$", l)
        if m:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                meta[rename.get(m.group(2), m.group(2))] = cur
    return funcs, meta


def main():
    show = "--diff" in sys.argv
    if show:
        sys.argv.remove("--diff")
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, old_meta = parse(sys.argv[1], RENAMED)
    new, new_meta = parse(sys.argv[2], {})
    bad = 0
    for name in sorted(set(old) | set(new), key=lambda n: (n not in old_meta and n not in new_meta, n)):
        kind = "kernel" if name in old_meta or name in new_meta else "function"
        if name not in old or name not in new:
            print(f"{kind} {name}: only in {'OLD' if name in old else 'NEW'}")
            bad += 1
            continue
        (a, na), (b, nb) = old[name], new[name]
        changed = sum(max(j1 - i1, j2 - i2) for op, i1, j1, i2, j2 in
                      difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if op != "equal") if a != b else 0
        fields = [f"instructions {na} -> {nb}"]
        if kind == "kernel":
            fields = [f"{k} {old_meta[name].get(k)} -> {new_meta[name].get(k)}" for k in META] + fields
            changed = changed or sum(old_meta[name].get(k) != new_meta[name].get(k) for k in META)
        if changed:
            bad += 1
            print(f"{kind} {name}: {changed} lines differ; " + ", ".join(fields))
            if show:
                print("\n".join(difflib.unified_diff(a, b, "OLD", "NEW", lineterm="", n=2)))
        else:
            print(f"{kind} {name}: identical ({nb} instructions)")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
