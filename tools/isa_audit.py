#!/usr/bin/env python3
"""Resources and hot-block instruction mix of EVERY kernel in two sets of gfx950 assembly files, side by side (no GPU needed).

    hipcc ... --cuda-device-only -S   (or EXTRA=--save-temps) for both builds, the .s files of each in one directory
    python tools/isa_audit.py BEFORE_DIR AFTER_DIR [--json profiles/NAME.json] [--only zf_trial_ zf_solver ...]

Per kernel (matched by mangled name): VGPRs, waves per SIMD (512 / VGPRs rounded up to 8), LDS, scratch - as
tools/kernel_resources.py - and, for the basic block with the most fp64 VALU instructions - as tools/isa_mix.py -
its VALU / fp64 / v_bfi_b32 / v_min_f64 / v_max_f64 counts.  Every soft-threshold of the fused element bodies ends in exactly one v_bfi_b32
(csrc/zf_common.h: zf_soft_threshold_nn), so in a block that only runs those bodies VALU / v_bfi and fp64 / v_bfi are
the instructions per element and trial (or replayed iteration).  The exit status is 1 if a kernel lost a wave per
SIMD or acquired scratch."""
from __future__ import annotations

import argparse
import collections
import glob
import json
import os
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
        return dict(zip(names, out)) if len(out) == len(names) else {n: n for n in names}
    except OSError:
        return {n: n for n in names}


def kernels_of(path):
    """{mangled name: record} for one assembly file."""
    text = open(path).read()
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        name, body = m.group(1), m.group(2)
        g = lambda k: int(re.search(rf"\.amdhsa_{k} (\d+)", body).group(1))   # noqa: E731
        vg = g("next_free_vgpr")
        res[name] = dict(vgpr=vg, waves_per_simd=min(512 // ((vg + 7) // 8 * 8), 8) if vg else 8,
                         lds=g("group_segment_fixed_size"), scratch=g("private_segment_fixed_size"))
    lines = text.splitlines()
    for name, rec in res.items():
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        blocks, cur = [], []
        for ln in lines[start + 1:]:
            s = ln.strip()
            if s.startswith(".Lfunc_end"):
                break
            if re.match(r"^\.?[A-Za-z_0-9$]+:", s):   # a label: the next basic block
                blocks.append(cur)
                cur = []
            elif s and not s.startswith((";", ".")):
                cur.append(s.split()[0])
        blocks.append(cur)
        f64 = lambda ops: sum(1 for o in ops if o.startswith("v_") and "f64" in o)   # noqa: E731
        hot = max(blocks, key=f64)
        h = collections.Counter(hot)
        valu = sum(c for o, c in h.items() if o.startswith("v_"))
        rec["hot_block"] = dict(valu=valu, f64=f64(hot), bfi=h.get("v_bfi_b32", 0), v_min_f64=h.get("v_min_f64", 0),
                                v_max_f64=h.get("v_max_f64", 0), s_nop=h.get("s_nop", 0))
        if h.get("v_bfi_b32", 0) >= 8:
            rec["hot_block"]["valu_per_bfi"] = round(valu / h["v_bfi_b32"], 3)
            rec["hot_block"]["f64_per_bfi"] = round(f64(hot) / h["v_bfi_b32"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--json")
    ap.add_argument("--only", nargs="*", default=[], help="file-name prefixes to keep (default: every .s file)")
    ap.add_argument("--note", default="")
    a = ap.parse_args()
    table, bad = {}, []
    for fa in sorted(glob.glob(os.path.join(a.after, "*.s"))):
        base = os.path.basename(fa)
        unit = base.split("-hip-")[0].replace(".s", "")
        if a.only and not any(unit.startswith(p) for p in a.only):
            continue
        fb = os.path.join(a.before, base)
        kb, ka = kernels_of(fb), kernels_of(fa)
        names = demangle(sorted(ka))
        rows = {}
        for n in sorted(ka):
            short = re.sub(r"\(zf_step_args.*", "", names[n]).replace("void ", "")
            b, k = kb.get(n), ka[n]
            rows[short] = dict(before=b, after=k)
            if b and (k["waves_per_simd"] < b["waves_per_simd"] or (k["scratch"] > 0 and b["scratch"] == 0)):
                bad.append(short)
        table[unit] = rows
    n_k = sum(len(r) for r in table.values())
    changed = sum(1 for r in table.values() for v in r.values() if v["before"] and v["before"] != v["after"])
    out = dict(note=a.note, kernels=n_k, kernels_changed=changed, lost_a_wave_or_gained_scratch=bad, units=table)
    txt = json.dumps(out, indent=1)
    if a.json:
        open(a.json, "w").write(txt + "\n")
    for unit, rows in table.items():
        for short, v in rows.items():
            b, k = v["before"], v["after"]
            if not b or b == k:
                continue
            hb, hk = b["hot_block"], k["hot_block"]
            print(f"{unit:28s} {short[:70]:70s} vgpr {b['vgpr']:3d}->{k['vgpr']:3d} waves {b['waves_per_simd']}->{k['waves_per_simd']} "
                  f"scratch {b['scratch']}->{k['scratch']}  valu/bfi {hb.get('valu_per_bfi')}->{hk.get('valu_per_bfi')} "
                  f"f64/bfi {hb.get('f64_per_bfi')}->{hk.get('f64_per_bfi')}")
    print(f"{n_k} kernels, {changed} changed, {len(bad)} lost a wave per SIMD or gained scratch: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
