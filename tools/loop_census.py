"""Static instruction census of the loops of one kernel in a gfx950 assembly listing.

    hipcc <the Makefile's flags> --offload-device-only -S csrc/rt_inw_fold.hip -o k.s
    python tools/loop_census.py k.s 'k_inw_pmILb0ELb1ELb1ELb1ELb0' [--has buffer_load_dwordx4=7] [--cut global_load]

A loop is the text from a label to a later branch back to it.  Every loop of the kernel is listed
with its depth and its count per instruction class, by mnemonic prefix only: v_ VALU, s_waitcnt,
s_nop, s_cbranch / s_branch, s_load / s_buffer_load SMEM, other s_ SALU, buffer_ / global_ / flat_ /
scratch_ VMEM, ds_ LDS.  --has MNEMONIC=N keeps the loops holding exactly N of that mnemonic outside
their inner loops.  --cut MNEMONIC leaves out of a loop's count the inner regions that a forward
branch skips and that hold the mnemonic (the wide walk's leaf batch, between its `s_cbranch` and
the label it jumps to, holds the trip's only global loads).
"""
import argparse
import re
import sys

CLASSES = ("VALU", "SALU", "branch", "s_waitcnt", "s_nop", "SMEM", "VMEM", "LDS", "other")


def classify(m):
    if m.startswith("v_"):
        return "VALU"
    if m.startswith("s_waitcnt"):
        return "s_waitcnt"
    if m == "s_nop":
        return "s_nop"
    if m.startswith("s_cbranch") or m == "s_branch":
        return "branch"
    if m.startswith("s_load") or m.startswith("s_buffer_load"):
        return "SMEM"
    if m.startswith("s_"):
        return "SALU"
    if m.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "VMEM"
    if m.startswith("ds_"):
        return "LDS"
    return "other"


def kernel_lines(path, pat):
    rx = re.compile(pat)
    out, on, name = [], False, None
    for ln in open(path):
        s = ln.split(";")[0].strip()
        if not on:
            if s.endswith(":") and not s.startswith(".") and rx.search(s):
                on, name = True, s[:-1]
            continue
        if s.startswith(".end_amdhsa_kernel") or s.startswith(".Lfunc_end"):
            break
        if not s or s.startswith((";", "//")):
            continue
        out.append(s.split(";")[0].strip())
    if name is None:
        raise SystemExit(f"no kernel matches {pat}")
    return name, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--has", default="")
    ap.add_argument("--cut", default="")
    a = ap.parse_args()
    name, L = kernel_lines(a.asm, a.kernel)
    label = {}
    for i, s in enumerate(L):
        if s.endswith(":"):
            label[s[:-1]] = i
    is_ins = [not (s.endswith(":") or s.startswith(".")) for s in L]
    mn = [s.split()[0] if is_ins[i] else "" for i, s in enumerate(L)]
    tgt = [None] * len(L)
    for i, s in enumerate(L):
        if classify(mn[i]) == "branch":
            t = s.split()[-1]
            tgt[i] = label.get(t)
    loops = sorted({(tgt[i], i) for i in range(len(L)) if tgt[i] is not None and tgt[i] <= i})
    # one loop per header: its last back edge
    by_head = {}
    for h, e in loops:
        by_head[h] = max(e, by_head.get(h, e))
    loops = sorted(by_head.items())
    want_m, want_n = (a.has.split("=") + ["0"])[:2] if a.has else ("", "0")
    print(name)
    print(f"{'lines':>13} depth " + " ".join(f"{c:>9}" for c in CLASSES) + "     total")
    for h, e in loops:
        depth = sum(1 for h2, e2 in loops if h2 <= h and e <= e2)
        inner = [(h2, e2) for h2, e2 in loops if h < h2 and e2 <= e or (h <= h2 and e2 < e)]
        skip = set()
        for h2, e2 in inner:
            skip.update(range(h2, e2 + 1))
        if a.cut:
            for i in range(h, e + 1):
                if tgt[i] is not None and i < tgt[i] <= e and any(mn[j].startswith(a.cut) for j in range(i + 1, tgt[i])):
                    skip.update(range(i + 1, tgt[i]))
        cnt = dict.fromkeys(CLASSES, 0)
        nm = 0
        for i in range(h, e + 1):
            if not is_ins[i] or i in skip:
                continue
            cnt[classify(mn[i])] += 1
            nm += mn[i] == want_m
        if a.has and nm != int(want_n):
            continue
        print(f"{h:>6}-{e:<6} {depth:>5} " + " ".join(f"{cnt[c]:>9}" for c in CLASSES) + f" {sum(cnt.values()):>9}")


if __name__ == "__main__":
    sys.exit(main())
