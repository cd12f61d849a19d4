#!/usr/bin/env python3
"""Where the line tail kernel (mgk_tail_cycle_line_f64) spends its time: (s_memrealtime, s_memtime) stamps at each of
its barriers (mgk_debug_tail_stamps), summed per kind of phase and per level.
usage: line_tail_phases.py [yline|xline|altline] [--uniform] [--n0 63] [--out FILE]
Random diagonally dominant row tables (the time of a phase does not depend on the values); --uniform: the x tables in the stride-0 form of the
uniform mesh (one row, kept in LDS) instead of n x n tables read from global memory."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import line_reference as LR  # noqa: E402
import xline_reference as XR  # noqa: E402
from row_tables import _rt_tables  # noqa: E402
from multigrid_petsc_amd.mgk import Mgk  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("pc", nargs="?", default="altline", choices=["yline", "xline", "altline"])
ap.add_argument("--uniform", action="store_true")
ap.add_argument("--n0", type=int, default=63)
ap.add_argument("--out", default=None)
a = ap.parse_args()
pc = {"yline": 1, "xline": 2, "altline": 3}[a.pc]
v = (3, 3)

m = Mgk(0)
L = m.L
ns = [a.n0]
while ns[-1] > 1:
    ns.append((ns[-1] - 1) // 2)
tabs = {k: [] for k in ("ctab", "ltab", "gtab", "qtab", "xgtab")}
xgs = []
for n in ns:
    ct = _rt_tables(np.random.default_rng(n + 1), n)[0]
    if a.uniform:
        ct = np.tile(ct[min(1, n - 1)], (n, 1))
    l, g, q = LR.tables(ct)
    gs = 0 if a.uniform else (n + 15) // 16 * 16
    xg = np.zeros((1 if a.uniform else n, (n + 15) // 16 * 16))
    xg[:, :n] = XR.table(ct[:1] if a.uniform else ct, n)
    for k, arr in zip(tabs, (ct, l, g, q, xg.ravel())):
        tabs[k].append(m.upload(arr))
    xgs.append(gs)
g0 = m.geom(2, ns[0])
b = m.to_field(g0, np.random.default_rng(0).uniform(-1, 1, ns[0] ** 2))
u = m.field(g0)
stamps = m.alloc(8 * 257)
L.mgk_debug_tail_stamps(stamps)
for rep in range(3):
    m._chk(m.tail_cycle_line(g0, ns, pc, scale=0.8, v=v, b=b, u=u, xgs=xgs, **tabs))
m.sync()
L.mgk_debug_tail_stamps(None)
raw = np.empty(257, dtype=np.int64)
m._chk(L.mgk_d2h(m.ctx, raw.ctypes.data_as(C.c_void_p), stamps, raw.nbytes))

# the kernel's phases in its own order: one label per stamp after the first
labels = [("setup", -1), ("load b", 0)]
nl = len(ns)
for stg in range(2 * nl - 1):
    down = stg < nl
    lv = stg if down else 2 * nl - 2 - stg
    if down and lv > 0:
        labels += [("residual", lv - 1), ("restrict", lv)]
    if not down:
        labels.append(("prolong", lv))
    for k in range(v[1] if (down and lv == nl - 1) else v[0]):
        isx = pc == 2 or (pc == 3 and k % 2 == 1)
        if not (down and k == 0):
            labels.append(("residual", lv))
        labels.append(("x march" if isx else "y march", lv))
labels.append(("store u", 0))
k = int(raw[256])
wall, clk = raw[0:2 * k:2], raw[1:2 * k:2]
assert k == len(labels) + 1 or k == 128, (k, len(labels))
total = (wall[-1] - wall[0]) / 100
ghz = (clk[-1] - clk[0]) / total / 1e3
print(f"{a.pc}{' uniform' if a.uniform else ''}: levels {ns}: {k} stamps, total {total:.2f} us, shader clock {ghz:.2f} GHz")
kinds, per_level = {}, {}
for i in range(1, k):
    kind, lv = labels[i - 1]
    us = (wall[i] - wall[i - 1]) / 100
    kinds[kind] = kinds.get(kind, 0.0) + us
    if lv >= 0:
        per_level[ns[lv]] = per_level.get(ns[lv], 0.0) + us
    print(f"  phase {i:3d}: {kind:9s} n = {ns[lv] if lv >= 0 else 0:2d}  {us:6.2f} us  {clk[i] - clk[i - 1]:7d} clk")
print("  by kind: " + ", ".join(f"{kk} {vv:.2f}" for kk, vv in kinds.items()))
print("  by level: " + ", ".join(f"n={kk} {vv:.2f}" for kk, vv in per_level.items()))
if a.out:
    with open(a.out, "a") as fo:
        fo.write(json.dumps({"pc": a.pc, "uniform": a.uniform, "levels": ns, "v": v, "stamps": k, "total_us": total, "shader_ghz": ghz,
                             "us_by_kind": kinds, "us_by_level": {str(kk): vv for kk, vv in per_level.items()},
                             "phases": [[labels[i - 1][0], ns[labels[i - 1][1]] if labels[i - 1][1] >= 0 else 0, (int(wall[i] - wall[i - 1])) / 100,
                                         int(clk[i] - clk[i - 1])] for i in range(1, k)]}) + "\n")
m.close()
