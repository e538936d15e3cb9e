#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly files (hipcc ... --cuda-device-only -S on the same source at two commits).

    asm_kernel_diff.py BEFORE.s AFTER.s [--family NAME ...] [--table]

For every kernel: identical text between the kernel's label and its .Lfunc_end, or not.  For a kernel that differs: VGPRs, SGPRs, LDS
bytes, scratch bytes and the length in instructions of every loop body (the instructions a backward branch spans, in the order of the
branches), before and after.  A kernel named by --family (a substring of its demangled or mangled name) may differ as long as no
resource figure and no loop body grew; any other kernel must be identical.  Exit status 1 when that does not hold.  --table prints the
figures of the family's kernels in AFTER.s.
Either file may be the concatenation of several translation units' assemblies (cat unit1.s unit2.s ...): kernels are found by name.
"""
import argparse
import re
import subprocess
import sys

FIG = (("VGPR", r"; NumVgprs: (\d+)"), ("SGPR", r"; TotalNumSgprs: (\d+)"), ("LDS", r"; LDSByteSize: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"))


def kernels(path):
    lines = open(path).read().split("\n")
    names = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel (\S+)", ln)] if m]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        # the number of the function inside its labels moves with the file, not with the kernel (template kernels are emitted behind
        # every plain one, so a new plain kernel renumbers them; the loop comments name the header as BB<n>_<m>, without the .L)
        # ... and the comment column is padded after the label as written, a digit more or less
        body = [re.sub(r"\s+;", " ;", re.sub(r"\bBB\d+_", "BB_", re.sub(r"\.LBB\d+_", ".LBB_", ln))) for ln in lines[start + 1:end]]
        info = {}
        for i in range(end, len(lines)):
            for key, pat in FIG:
                m = re.match(pat, lines[i])
                if m and key not in info:
                    info[key] = int(m.group(1))
            if len(info) == len(FIG):
                break
        out[name] = (body, info, loops(body))
    return out


def loops(body):
    """Lengths of the loop bodies: for every branch to a label above it, the instructions from the label to the branch."""
    label_at, count, res = {}, 0, []
    for ln in body:
        text = ln.split(";")[0].strip()
        if not text:
            continue
        m = re.match(r"(\.LBB_\d+):", text)
        if m:
            label_at[m.group(1)] = count
            continue
        if text.startswith("."):
            continue
        count += 1
        m = re.match(r"s_c?branch\S*\s+(\.LBB_\d+)", text)
        if m and m.group(1) in label_at:
            res.append(count - label_at[m.group(1)])
    return res


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--family", action="append", default=[])
    ap.add_argument("--table", action="store_true")
    a = ap.parse_args()
    kb, ka = kernels(a.before), kernels(a.after)
    pretty = demangle(sorted(set(kb) | set(ka)))
    bad = 0
    for name in sorted(set(kb) | set(ka), key=lambda n: pretty[n]):
        short = pretty[name].split("(")[0]
        fam = any(f in pretty[name] or f in name for f in a.family)
        if name not in kb or name not in ka:
            print("MISSING  %s (%s)" % (short, "before" if name not in kb else "after"))
            bad += 1
            continue
        (tb, ib, lb), (ta, ia, la) = kb[name], ka[name]
        if tb == ta and ib == ia:
            if fam:
                print("same     %s" % short)
            continue
        grew = [k for k, _ in FIG if ia[k] > ib[k]]
        if len(la) != len(lb):
            grew.append("loops %d -> %d" % (len(lb), len(la)))
        else:
            grew += ["loop %d: %d -> %d" % (i, x, y) for i, (x, y) in enumerate(zip(lb, la)) if y > x]
        ok = fam and not grew
        bad += not ok
        print("%s %s\n    before %s loops %s\n    after  %s loops %s%s" % ("differs " if ok else "WORSE   " if fam else "MOVED   ", short, ib, lb, ia, la,
                                                                        "\n    grew: " + ", ".join(grew) if grew else ""))
    if a.table:
        print("\n| kernel | VGPR | SGPR | LDS bytes | scratch | loop bodies (instructions) |\n|---|---|---|---|---|---|")
        for name in sorted(ka, key=lambda n: pretty[n]):
            if any(f in pretty[name] or f in name for f in a.family):
                _, i, l = ka[name]
                print("| `%s` | %d | %d | %d | %d | %s |" % (pretty[name].split("(")[0], i["VGPR"], i["SGPR"], i["LDS"], i["scratch"], ", ".join(map(str, l))))
    print("%d kernels before, %d after, %d not acceptable" % (len(kb), len(ka), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
