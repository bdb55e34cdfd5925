"""Opcode histogram of the loops of a kernel that hold matrix instructions, from hipcc's assembly listing.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S ecg_denoise_amd/csrc/ral_attnm.hip -o attnm.s
    python tools/diag/loop_isa_hist.py attnm.s k_attn_bwd_mhILi4ELb0 [k_attn_bwd_mILi128ELb1 ...]

A loop is the span from a label to the LAST backward branch to it; only innermost spans with matrix instructions are
printed (the tile sweeps: one per scaling mode).  Counts are static: with a table the span holds both sides of the
per-tile test, so the table side's instructions are listed too (the `scalar` and `branch` lines show how many)."""
import collections
import re
import sys


def functions(path):
    name, body, out = None, [], {}
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            out[name] = body
        elif line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            name = None
        elif name:
            body.append(line.rstrip("\n"))
    return out


def loops(body):
    labels = {}
    spans = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
        m = re.match(r"^\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.match(r"^\s+s_branch\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels:
            spans[labels[m.group(1)]] = i
    spans = sorted(spans.items())
    inner = [s for s in spans if not any(t != s and s[0] <= t[0] and t[1] <= s[1] for t in spans
                                         if any("v_mfma" in x for x in body[t[0]:t[1]]))]
    return [s for s in inner if any("v_mfma" in x for x in body[s[0]:s[1]])]


def hist(lines):
    h = collections.Counter()
    for l in lines:
        m = re.match(r"^\s+([a-z_0-9]+)", l)
        if m and not l.lstrip().startswith((";", ".")):
            h[m.group(1)] += 1
    return h


def main():
    fns = functions(sys.argv[1])
    for want in sys.argv[2:]:
        for name, body in fns.items():
            if want not in name:
                continue
            for a, b in loops(body):
                h = hist(body[a:b + 1])
                mfma = sum(n for k, n in h.items() if k.startswith("v_mfma"))
                nop = h.get("s_nop", 0)
                vec = sum(n for k, n in h.items() if k.startswith("v_") and not k.startswith("v_mfma"))
                lds = sum(n for k, n in h.items() if k.startswith("ds_"))
                br = sum(n for k, n in h.items() if k.startswith(("s_cbranch", "s_branch")))
                sc = sum(n for k, n in h.items() if k.startswith("s_")) - nop - br
                scr = sum(n for k, n in h.items() if k.startswith("scratch_"))
                print(f"{name}  loop of {b - a + 1} lines: vector (non-matrix) {vec}, matrix {mfma}, s_nop {nop}, "
                      f"LDS {lds}, scalar {sc}, branch {br}, scratch {scr}")
                for k, n in sorted(h.items(), key=lambda kv: (-kv[1], kv[0])):
                    if k.startswith(("v_", "ds_")):
                        print(f"    {n:4d}  {k}")


if __name__ == "__main__":
    main()
