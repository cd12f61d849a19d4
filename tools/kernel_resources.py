#!/usr/bin/env python3
"""Register / scratch figures of the k_jacobi3_2d and k_tail* instances, read from hipcc's -Rpass-analysis=kernel-resource-usage remarks
(no GPU needed):  hipcc ... -Rpass-analysis=kernel-resource-usage -c mgk_sweep3.hip 2> log;  tools/kernel_resources.py log [name-filter]"""
import re
import sys


def rows(path):
    out, cur = [], None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: (.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = {"name": t.split(":", 1)[1].strip()}
            out.append(cur)
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    return out


def pretty(mangled):
    m = re.match(r"_Z\d+(k_\w+?)I(.*)E+v", mangled)
    if not m:
        return mangled
    args = re.findall(r"L([bi])(\d+)E|([df])", m.group(2))
    txt = [("double" if c == "d" else "float") if c else (v if k == "i" else ("T" if v == "1" else "F")) for k, v, c in args]
    return f"{m.group(1)}<{','.join(txt)}>"


if __name__ == "__main__":
    flt = sys.argv[2] if len(sys.argv) > 2 else "k_"
    print("| kernel | VGPRs | AGPRs | SGPRs | scratch B/lane | waves/SIMD |")
    print("|---|---|---|---|---|---|")
    for r in rows(sys.argv[1]):
        if flt in r["name"]:
            print(f"| {pretty(r['name'])} | {r.get('VGPRs')} | {r.get('AGPRs')} | {r.get('TotalSGPRs')} | {r.get('ScratchSize [bytes/lane]')} | {r.get('Occupancy [waves/SIMD]')} |")
