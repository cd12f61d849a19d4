"""Recorded reference output (tests/golden/ref_maps.npz, ref_assembly.npz): the case lists, the parser of oracle/_ref/record's lines, the
packing into the committed arrays and the views the tests read.  Test infrastructure only.

The two files hold numbers alone (int32 / float64, allow_pickle=False).  Every case's arrays lie one after the other in a few long arrays, in
the order of `cases`; the views below cut them apart again.

ref_maps.npz      cases (N x 5: npts grids levels map procs), levgrids / levtotal (per level), gridid, h (per grid x 2), ranges, glob, grid;
                  rcases / rranges: the cases of which only the ranges are kept
ref_assembly.npz  cases (N x 6: mesh npts grids levels map full), mesh_h, coord (2 npts per case), h, res0 / pro0 (N x 9, zero where one grid),
                  error (N x 3: GetError on U1), ncalls (N) and the stream obj row col val mode in call order; obj = 32 * kind + level with
                  kind 0 A, 1 res, 2 pro, 3 b.  full == 0: the right-hand side alone (the matrix calls are dropped)."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RECORD = os.path.join(ROOT, "oracle", "_ref", "record")
MAPS_NPZ = os.path.join(HERE, "golden", "ref_maps.npz")
ASSEMBLY_NPZ = os.path.join(HERE, "golden", "ref_assembly.npz")
ADD_VALUES, INSERT_VALUES = 2, 1
KIND_A, KIND_R, KIND_P, KIND_B = 0, 1, 2, 3

MAP_SHAPES = [(9, 2, 2), (17, 3, 3), (33, 4, 4), (33, 5, 5), (9, 3, 1), (17, 3, 1), (17, 3, 2), (33, 4, 2), (33, 4, 3)]
MAP_CASES = [(n, g, l, m, p) for (n, g, l) in MAP_SHAPES for m in (0, 1, 2) for p in (1, 2, 3, 4, 8)]
# ranges alone: the issue's (129, 6, 6) at 8 ranks, and the shapes of vcycle_golden.npz's ranges_n*_p* that the list above lacks
RANGES_CASES = [(129, 6, 6, 2, 8)] + [(n, l, l, 2, p) for (n, l) in ((9, 3), (17, 4)) for p in (1, 2, 4, 8)]
ASSEMBLY_SHAPES = [(9, 2, 2, 2), (17, 3, 3, 2), (33, 4, 4, 2), (17, 3, 2, 0), (17, 3, 2, 1), (17, 3, 2, 2), (17, 3, 1, 2)]
ASSEMBLY_CASES = [(mesh, n, g, l, m, 1) for mesh in (0, 1, 2) for (n, g, l, m) in ASSEMBLY_SHAPES] + \
                 [(mesh, n, 1, 1, 2, 0) for mesh in (0, 1, 2) for n in (65, 129)]


def U1(npts):
    """the deterministic field GetError is recorded on"""
    i, j = np.meshgrid(np.arange(npts - 2), np.arange(npts - 2), indexing="ij")
    return ((7 * i + 3 * j) % 11) / 11.0


def record(npts, grids, levels, style, mesh, procs, rank=0):
    """one run of the recorder, parsed: {tag: [fields, ...]} with the doubles exact (float.fromhex)"""
    p = subprocess.run([RECORD] + [str(v) for v in (npts, grids, levels, style, mesh, procs, rank)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    if p.returncode != 0:
        raise RuntimeError(f"record failed ({p.returncode}): {p.stderr[-2000:]}")
    out = {}
    for line in p.stdout.splitlines():
        f = line.split()
        if f and f[0] in ("mesh_h", "coord", "level", "gridid", "h", "ranges", "global", "grid", "res", "pro", "call", "handle", "error"):
            out.setdefault(f[0], []).append(f[1:])
    return out


def _ints(f):
    return np.array([int(v) for v in f], dtype=np.int32)


def _dbls(f):
    return np.array([float.fromhex(v) for v in f], dtype=np.float64)


def _level_arrays(rec):
    levgrids = _ints([f[1] for f in rec["level"]])
    levtotal = _ints([f[2] for f in rec["level"]])
    gridid = np.concatenate([_ints(f[1:]) for f in rec["gridid"]])
    h = np.array([_dbls(f[2:]) for f in rec["h"]]).reshape(-1, 2)
    ranges = np.concatenate([_ints(f[1:]) for f in rec["ranges"]])
    glob = np.concatenate([_ints(f[1:]) for f in rec["global"]])
    grid = np.concatenate([_ints(f[4:]) for f in rec["grid"]])
    return levgrids, levtotal, gridid, h, ranges, glob, grid


def build_maps():
    """run the recorder over MAP_CASES / RANGES_CASES -> the arrays of ref_maps.npz"""
    parts = {k: [] for k in ("levgrids", "levtotal", "gridid", "h", "ranges", "glob", "grid")}
    for (n, g, l, m, p) in MAP_CASES:
        for k, a in zip(parts, _level_arrays(record(n, g, l, m, 0, p))):
            parts[k].append(a)
    out = {k: np.concatenate(v) for k, v in parts.items()}
    out["cases"] = np.array(MAP_CASES, dtype=np.int32)
    out["rcases"] = np.array(RANGES_CASES, dtype=np.int32)
    out["rranges"] = np.concatenate([_level_arrays(record(n, g, l, m, 0, p))[4] for (n, g, l, m, p) in RANGES_CASES])
    return out


def build_assembly():
    """run the recorder over ASSEMBLY_CASES -> the arrays of ref_assembly.npz"""
    parts = {k: [] for k in ("mesh_h", "coord", "h", "res0", "pro0", "error", "ncalls", "obj", "row", "col", "val", "mode")}
    for (mesh, n, g, l, m, full) in ASSEMBLY_CASES:
        rec = record(n, g, l, m, mesh, 1)
        name = {int(f[0]): 32 * int(f[1]) + int(f[2]) for f in rec["handle"]}
        calls = [f for f in rec["call"] if full or f[0] == "V"]
        obj = np.array([name[int(f[1])] for f in calls], dtype=np.int32)
        parts["mesh_h"].append(_dbls(rec["mesh_h"][0]))
        parts["coord"].append(np.concatenate([_dbls(f[2:]) for f in rec["coord"]]))
        parts["h"].append(np.array([_dbls(f[2:]) for f in rec["h"]]).reshape(-1, 2))
        parts["res0"].append(_dbls(rec["res"][0][3:]) if g > 1 else np.zeros(9))
        parts["pro0"].append(_dbls(rec["pro"][0][3:]) if g > 1 else np.zeros(9))
        parts["error"].append(_dbls(rec["error"][0]))
        parts["ncalls"].append(np.array([len(calls)], dtype=np.int32))
        parts["obj"].append(obj)
        parts["row"].append(_ints([f[2] for f in calls]))
        parts["col"].append(_ints([f[3] for f in calls]))
        parts["val"].append(_dbls([f[4] for f in calls]))
        parts["mode"].append(_ints([f[5] for f in calls]))
    out = {k: np.concatenate(v) for k, v in parts.items()}
    for k in ("res0", "pro0", "error"):
        out[k] = out[k].reshape(len(ASSEMBLY_CASES), -1)
    out["cases"] = np.array(ASSEMBLY_CASES, dtype=np.int32)
    return out


# ---- views of the committed files ----
def _grid_n(npts, g):
    return (npts - 1) // 2 ** g - 1


def load_maps(arrays=None):
    """{(npts, grids, levels, map, procs): {grids, total, gridid, h, ranges [levels x procs+1], glob [per level: total x 3], grid [per level: list
    of ni x nj]}}, and {case: ranges} of the ranges-only cases"""
    z = dict(np.load(MAPS_NPZ, allow_pickle=False)) if arrays is None else arrays
    out, ol, og, orr, ogl, ogr = {}, 0, 0, 0, 0, 0
    for case in map(tuple, z["cases"].tolist()):
        npts, grids, levels, _, procs = case
        lg = z["levgrids"][ol:ol + levels]
        tot = z["levtotal"][ol:ol + levels]
        ng = int(lg.sum())
        c = {"grids": lg, "total": tot, "gridid": z["gridid"][og:og + ng], "h": z["h"][og:og + ng],
             "ranges": z["ranges"][orr:orr + levels * (procs + 1)].reshape(levels, procs + 1), "glob": [], "grid": []}
        q = 0
        for l in range(levels):
            c["glob"].append(z["glob"][ogl:ogl + 3 * int(tot[l])].reshape(-1, 3))
            ogl += 3 * int(tot[l])
            per = []
            for _ in range(int(lg[l])):
                n = _grid_n(npts, int(c["gridid"][q]))
                per.append(z["grid"][ogr:ogr + n * n].reshape(n, n))
                ogr += n * n
                q += 1
            c["grid"].append(per)
        ol += levels; og += ng; orr += levels * (procs + 1)
        out[case] = c
    assert (ol, og, orr, ogl, ogr) == (len(z["levgrids"]), len(z["gridid"]), len(z["ranges"]), len(z["glob"]), len(z["grid"]))
    ronly, o = {}, 0
    for case in map(tuple, z["rcases"].tolist()):
        k = case[2] * (case[4] + 1)
        ronly[case] = z["rranges"][o:o + k].reshape(case[2], case[4] + 1)
        o += k
    assert o == len(z["rranges"])
    return out, ronly


def load_assembly(arrays=None):
    """{(mesh, npts, grids, levels, map, full): {mesh_h, coord [2 x npts], h, res0, pro0 [3 x 3], error, obj, row, col, val, mode}}"""
    z = dict(np.load(ASSEMBLY_NPZ, allow_pickle=False)) if arrays is None else arrays
    out, oc, oh, os_ = {}, 0, 0, 0
    for q, case in enumerate(map(tuple, z["cases"].tolist())):
        _, npts, grids, _, _, _ = case
        k = int(z["ncalls"][q])
        c = {"mesh_h": float(z["mesh_h"][q]), "coord": z["coord"][oc:oc + 2 * npts].reshape(2, npts), "h": z["h"][oh:oh + grids],
             "res0": z["res0"][q].reshape(3, 3), "pro0": z["pro0"][q].reshape(3, 3), "error": z["error"][q]}
        for name in ("obj", "row", "col", "val", "mode"):
            c[name] = z[name][os_:os_ + k]
        oc += 2 * npts; oh += grids; os_ += k
        out[case] = c
    assert (oc, oh, os_) == (len(z["coord"]), len(z["h"]), len(z["val"]))
    return out


def one_grid_per_level(case):
    """assembly case: full stream, -grids == -levels"""
    return case[5] == 1 and case[2] == case[3]


# ---- the stream as matrices and vectors ----
def stream_select(c, kind, level):
    sel = c["obj"] == 32 * kind + level
    return c["row"][sel], c["col"][sel], c["val"][sel], c["mode"][sel]


def stream_shape(c, kind, level, totals):
    """(rows, columns) of A[level] / res[level] / pro[level] from the level sizes"""
    return {KIND_A: (totals[level], totals[level]), KIND_R: (totals[min(level + 1, len(totals) - 1)], totals[level]),
            KIND_P: (totals[level], totals[min(level + 1, len(totals) - 1)])}[kind]


def stream_csr(c, kind, level, nrows):
    """what MatAssemblyEnd leaves of the recorded calls: per row the columns ascending, ADD_VALUES duplicates summed in call order (the first
    value of an entry is added to 0.0).  Returns (rowptr, col, val)."""
    row, col, val, mode = stream_select(c, kind, level)
    assert np.all(mode == ADD_VALUES) and row.size
    order = np.lexsort((np.arange(row.size), col, row))         # by row, then column, then call order
    r, cc, v = row[order], col[order], val[order]
    first = np.ones(r.size, dtype=bool)
    first[1:] = (r[1:] != r[:-1]) | (cc[1:] != cc[:-1])
    out_v = []
    for q in range(r.size):
        if first[q]:
            out_v.append(0.0 + float(v[q]))
        else:
            out_v[-1] = out_v[-1] + float(v[q])
    rowptr = np.zeros(nrows + 1, dtype=np.int64)
    np.add.at(rowptr, r[first].astype(np.int64) + 1, 1)
    return np.cumsum(rowptr), cc[first].astype(np.int32), np.array(out_v, dtype=np.float64)


def stream_vector(c, n=None):
    """b[0] as VecSetValue(INSERT_VALUES) leaves it: n values (default: as many as level 0 holds -- with several grids in level 0 the fine
    grid's (npts - 2)^2 are followed by the coarser grids' restricted values, src/solver.c:598-613)"""
    row, _, val, mode = stream_select(c, KIND_B, 0)
    n = row.size if n is None else n
    assert np.all(mode == INSERT_VALUES) and np.array_equal(np.sort(row), np.arange(n))
    b = np.zeros(n)
    b[row] = val
    return b


def csr_mult_canonical(rowptr, col, val, x):
    """the canonical product (oracle/mgo.h): columns ascending, separate multiply and add, the sum starts at 0.0"""
    y = np.zeros(len(rowptr) - 1)
    for r in range(len(y)):
        s = 0.0
        for k in range(rowptr[r], rowptr[r + 1]):
            s = s + float(val[k]) * float(x[col[k]])
        y[r] = s
    return y


# ---- comparisons (the teeth cases feed changed copies to the same helpers) ----
def same_bits(a, b):
    """equal shape, type and bit pattern (NaN-safe, distinguishes -0.0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_csr(got, want):
    """(rowptr, col, val) triples: the same pattern and the same bits"""
    kinds = (np.int64, np.int32, np.float64)
    return len(got) == len(want) == 3 and all(same_bits(np.asarray(g, dtype=k), np.asarray(w, dtype=k)) for g, w, k in zip(got, want, kinds))
