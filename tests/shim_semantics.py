"""PETSc semantics of the drop-in's lazy temporaries in call orders the reference's loop does not use.  Shared by the GPU
tier (the real libmgpetsc.so) and the CPU tier (petsc_shim.c over tests/mock_mgk.cpp, built by tests/test_shim_semantics_cpu.py): the
functions take the ctypes library `L` with its argument types set (`type_shim`)."""
import ctypes as C

import numpy as np

ADD, INSERT, FINAL, NORM_2 = 2, 1, 0, 1


def type_shim(L):
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    L.PetscInitialize.argtypes = [vp, vp, C.c_char_p, C.c_char_p]
    L.PetscOptionsSetValue.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.MatCreateAIJ.argtypes = [i, i, i, i, i, i, vp, i, vp, C.POINTER(vp)]
    L.MatSetValue.argtypes = [vp, i, i, d, i]
    L.MatAssemblyBegin.argtypes = [vp, i]
    L.MatAssemblyEnd.argtypes = [vp, i]
    L.MatCreateVecs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.MatMult.argtypes = [vp, vp, vp]
    L.MatResidual.argtypes = [vp, vp, vp, vp]
    L.MatDestroy.argtypes = [C.POINTER(vp)]
    L.VecSetValue.argtypes = [vp, i, d, i]
    L.VecAssemblyBegin.argtypes = [vp]
    L.VecAssemblyEnd.argtypes = [vp]
    L.VecDuplicate.argtypes = [vp, C.POINTER(vp)]
    L.VecSet.argtypes = [vp, d]
    L.VecCopy.argtypes = [vp, vp]
    L.VecScale.argtypes = [vp, d]
    L.VecAXPY.argtypes = [vp, d, vp]
    L.VecNorm.argtypes = [vp, i, C.POINTER(d)]
    L.VecGetArray.argtypes = [vp, C.POINTER(C.POINTER(d))]
    L.VecRestoreArray.argtypes = [vp, C.POINTER(C.POINTER(d))]
    L.VecDestroy.argtypes = [C.POINTER(vp)]
    L.KSPCreate.argtypes = [i, C.POINTER(vp)]
    L.KSPSetType.argtypes = [vp, C.c_char_p]
    L.KSPSetOperators.argtypes = [vp, vp, vp]
    L.KSPSetNormType.argtypes = [vp, i]
    L.KSPSetTolerances.argtypes = [vp, d, d, d, i]
    L.KSPSetFromOptions.argtypes = [vp]
    L.KSPSetInitialGuessNonzero.argtypes = [vp, i]
    L.KSPSolve.argtypes = [vp, vp, vp]
    L.KSPBuildResidual.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.KSPDestroy.argtypes = [C.POINTER(vp)]
    L.KSPRichardsonSetScale.argtypes = [vp, d]
    L.KSPGetPC.argtypes = [vp, C.POINTER(vp)]
    L.PCSetType.argtypes = [vp, C.c_char_p]
    L.PCMGSetLevels.argtypes = [vp, i, vp]
    L.PCMGGetCoarseSolve.argtypes = [vp, C.POINTER(vp)]
    L.PCMGGetSmoother.argtypes = [vp, i, C.POINTER(vp)]
    for f in (L.PCMGSetInterpolation, L.PCMGSetRestriction, L.PCMGSetR, L.PCMGSetRhs, L.PCMGSetX):
        f.argtypes = [vp, i, vp]
    return L


def _dense(orc, which, npts, l):
    m = orc.build(which, 2, npts, l)
    rows = orc.csr_rows(m)
    nr, nc = orc.L.mgo_csr_nrows(m), orc.L.mgo_csr_ncols(m)
    d = np.zeros((nr, nc))
    for r, (cols, vals) in enumerate(rows):
        d[r, list(cols)] = vals
    return d



def _assemble(L, M):
    m = C.c_void_p()
    L.MatCreateAIJ(1, M.shape[0], M.shape[1], -1, -1, 30, None, 0, None, C.byref(m))
    for r, c in zip(*np.nonzero(M)):
        L.MatSetValue(m, int(r), int(c), float(M[r, c]), ADD)
    L.MatAssemblyBegin(m, FINAL)
    L.MatAssemblyEnd(m, FINAL)
    return m



def _set(L, v, a):
    for q, val in enumerate(a):
        L.VecSetValue(v, q, float(val), INSERT)
    L.VecAssemblyBegin(v)
    L.VecAssemblyEnd(v)



def _get(L, v, n):
    p = C.POINTER(C.c_double)()
    L.VecGetArray(v, C.byref(p))
    a = np.ctypeslib.as_array(p, shape=(n,)).copy()
    L.VecRestoreArray(v, C.byref(p))
    return a




def lazy_temporaries_keep_petsc_semantics(L, orc):
    """the deferred residual / prolongation / correction vectors of the drop-in in call orders the reference's loop does
    NOT use: a deferred vector read later, an operand changed or destroyed before the deferred vector is read, a correction that no sweep
    follows -- every value must be what call-by-call execution gives"""
    L.PetscInitialize(None, None, None, None)
    npts = 33
    A, P, R = _dense(orc, "A", npts, 0), _dense(orc, "P", npts, 0), _dense(orc, "R", npts, 0)
    mA, mP, mR = _assemble(L, A), _assemble(L, P), _assemble(L, R)
    nf, nc = A.shape[0], P.shape[1]
    rng = np.random.default_rng(3)
    xv, bv, ucv = rng.standard_normal(nf), rng.standard_normal(nf), rng.standard_normal(nc)
    x, b, r, rv, u = (C.c_void_p() for _ in range(5))
    uc, bc = C.c_void_p(), C.c_void_p()
    L.MatCreateVecs(mA, C.byref(x), C.byref(b))
    for v in (r, rv, u):
        L.VecDuplicate(x, C.byref(v))
    L.MatCreateVecs(mR, None, C.byref(bc))
    L.MatCreateVecs(mP, C.byref(uc), None)
    tol = 1e-12 * np.abs(A).max() * 10
    _set(L, x, xv); _set(L, b, bv); _set(L, uc, ucv)
    # 1. a deferred residual whose operand changes before it is read: the OLD x counts
    L.MatResidual(mA, b, x, r)
    L.VecScale(x, 2.0)
    assert np.max(np.abs(_get(L, r, nf) - (bv - A @ xv))) <= tol
    assert np.max(np.abs(_get(L, x, nf) - 2.0 * xv)) == 0.0
    # 2. deferred residual consumed by the restriction AND read afterwards
    _set(L, x, xv)
    L.MatResidual(mA, b, x, r)
    L.MatMult(mR, r, bc)
    assert np.max(np.abs(_get(L, bc, nc) - R @ (bv - A @ xv))) <= tol
    assert np.max(np.abs(_get(L, r, nf) - (bv - A @ xv))) <= tol
    # 2b. the restricted right-hand side is deferred as well: its fine-level operands change before it is read
    L.MatResidual(mA, b, x, r)
    L.MatMult(mR, r, bc)
    L.VecScale(x, 2.0)
    L.VecSet(b, 0.0)
    assert np.max(np.abs(_get(L, bc, nc) - R @ (bv - A @ xv))) <= tol
    assert np.max(np.abs(_get(L, r, nf) - (bv - A @ xv))) <= tol
    _set(L, x, xv); _set(L, b, bv)
    # 3. deferred prolongation + deferred correction, no sweep follows: u and rv read directly
    _set(L, u, xv)
    L.MatMult(mP, uc, rv)
    L.VecAXPY(u, 1.0, rv)
    assert np.max(np.abs(_get(L, u, nf) - (xv + P @ ucv))) <= 1e-13 * 10
    assert np.max(np.abs(_get(L, rv, nf) - P @ ucv)) <= 1e-13 * 10
    # 4. the coarse operand changes between the deferred prolongation, the deferred correction and their use
    _set(L, u, xv)
    L.MatMult(mP, uc, rv)
    L.VecAXPY(u, 1.0, rv)
    L.VecScale(uc, -3.0)                       # both deferred values were defined with the old u_c
    assert np.max(np.abs(_get(L, u, nf) - (xv + P @ ucv))) <= 1e-13 * 10
    assert np.max(np.abs(_get(L, rv, nf) - P @ ucv)) <= 1e-13 * 10
    # 5. ... or is destroyed
    _set(L, uc, ucv); _set(L, u, xv)
    L.MatMult(mP, uc, rv)
    L.VecAXPY(u, 1.0, rv)
    L.VecDestroy(C.byref(uc))
    assert np.max(np.abs(_get(L, u, nf) - (xv + P @ ucv))) <= 1e-13 * 10
    # 6. a deferred vector that is copied, and one that is overwritten unread
    L.MatResidual(mA, b, x, r)
    L.VecCopy(r, rv)
    assert np.max(np.abs(_get(L, rv, nf) - (bv - A @ xv))) <= tol
    L.MatResidual(mA, b, x, r)
    L.VecSet(r, 7.0)
    assert np.all(_get(L, r, nf) == 7.0)
    for v in (x, b, r, rv, u, bc):
        L.VecDestroy(C.byref(v))
    for m in (mA, mP, mR):
        L.MatDestroy(C.byref(m))


def speculative_sweep_is_adopted_only_when_nothing_changed(L, orc):
    """KSPBuildResidual + VecNorm on a Richardson smoother with a nonzero guess also make the first sweep of the next KSPSolve (DESIGN.md 8b
    N2).  That sweep must be dropped when u or b is written between the norm and the solve, and adopted otherwise -- either way the
    iterate is what sweep-by-sweep execution gives."""
    L.PetscInitialize(None, None, None, None)
    L.PetscOptionsSetValue(None, b"-pc_type", b"jacobi")
    L.PetscOptionsSetValue(None, b"-ksp_richardson_scale", b"0.8")
    npts = 33
    A = _dense(orc, "A", npts, 0)
    mA = _assemble(L, A)
    n = A.shape[0]
    d = 1.0 / np.diag(A)
    rng = np.random.default_rng(11)
    uv, bv = rng.standard_normal(n), rng.standard_normal(n)
    u, b, r = C.c_void_p(), C.c_void_p(), C.c_void_p()
    L.MatCreateVecs(mA, C.byref(u), C.byref(b))
    L.VecDuplicate(u, C.byref(r))
    k = C.c_void_p()
    L.KSPCreate(1, C.byref(k))
    L.KSPSetType(k, b"richardson"); L.KSPSetOperators(k, mA, mA); L.KSPSetNormType(k, 0)
    L.KSPSetTolerances(k, 1e-7, -2.0, -2.0, 2)
    L.KSPSetFromOptions(k)
    L.KSPSetInitialGuessNonzero(k, 1)
    V, val = C.c_void_p(), C.c_double()

    def sweeps(x, rhs, m, s=0.8):
        for _ in range(m):
            x = x + s * (d * (rhs - A @ x))
        return x

    tol = 1e-12 * max(np.abs(uv).max(), 1.0) * 100
    # "scale" / "options": a PARAMETER of the solver changes between the norm and the solve: the sweep the norm pass made
    # with the old scale must be dropped, both sweeps of the next solve use the new one
    for change in ("nothing", "u", "b", "scale", "options"):
        _set(L, u, uv); _set(L, b, bv)
        L.KSPSolve(k, b, u)
        x = sweeps(uv, bv, 2)
        L.KSPBuildResidual(k, None, r, C.byref(V))
        L.VecNorm(V, NORM_2, C.byref(val))
        assert abs(val.value - np.linalg.norm(bv - A @ x)) <= 1e-12 * np.linalg.norm(bv - A @ x)
        rhs, s2 = bv, 0.8
        if change == "u":
            L.VecScale(u, 0.5); x = 0.5 * x
        if change == "b":
            L.VecScale(b, 2.0); rhs = 2.0 * bv
        if change == "scale":
            L.KSPRichardsonSetScale(k, 0.5); s2 = 0.5
        if change == "options":
            L.PetscOptionsSetValue(None, b"-ksp_richardson_scale", b"0.6")
            L.KSPSetFromOptions(k); s2 = 0.6
        L.KSPSolve(k, b, u)
        x2 = sweeps(x, rhs, 2, s2)
        if change in ("scale", "options"):          # back to the scale of the other rounds
            L.PetscOptionsSetValue(None, b"-ksp_richardson_scale", b"0.8")
            L.KSPRichardsonSetScale(k, 0.8)
        assert np.max(np.abs(_get(L, u, n) - x2)) <= tol, change
        assert np.max(np.abs(_get(L, r, n) - (bv - A @ sweeps(uv, bv, 2)))) <= tol * np.abs(A).max(), change     # r was stored by the norm pass
    L.KSPDestroy(C.byref(k))
    for v in (u, b, r):
        L.VecDestroy(C.byref(v))
    L.MatDestroy(C.byref(mA))


def residual_left_deferred_by_the_norm_pass(L, orc):
    """max_it = 3 (the reference's -v 3,3): the pass that evaluates || b - A u || makes ALL three sweeps of the next KSPSolve and does not
    store r (round 3): r stays deferred, and when the solve adopts the sweeps (x and the work vector swap buffers) r's dependency follows
    the OLD iterate into the work vector.  Whatever is done next -- r read at once, after the adopting solve, after b was rewritten, after
    another solve reused the work vector, after the solver died, the norm asked twice -- r must be b - A (old u) and u three sweeps further."""
    L.PetscInitialize(None, None, None, None)
    L.PetscOptionsSetValue(None, b"-pc_type", b"jacobi")
    L.PetscOptionsSetValue(None, b"-ksp_richardson_scale", b"0.8")
    npts = 33
    A = _dense(orc, "A", npts, 0)
    mA = _assemble(L, A)
    n = A.shape[0]
    d = 1.0 / np.diag(A)
    rng = np.random.default_rng(17)
    uv, bv = rng.standard_normal(n), rng.standard_normal(n)

    def sweeps(x, rhs, m, s=0.8):
        for _ in range(m):
            x = x + s * (d * (rhs - A @ x))
        return x

    tol = 1e-12 * max(np.abs(uv).max(), 1.0) * 100
    rtol = tol * np.abs(A).max()
    for case in ("reference order", "read r at once", "read r after the solve", "b rewritten after the solve", "second solve reuses the work vector",
                 "solver destroyed", "norm twice", "norm again after the solve", "u written before the solve", "restriction of r after the solve"):
        u, b, r = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.MatCreateVecs(mA, C.byref(u), C.byref(b))
        L.VecDuplicate(u, C.byref(r))
        k = C.c_void_p()
        L.KSPCreate(1, C.byref(k))
        L.KSPSetType(k, b"richardson"); L.KSPSetOperators(k, mA, mA); L.KSPSetNormType(k, 0)
        L.KSPSetTolerances(k, 1e-7, -2.0, -2.0, 3)
        L.KSPSetFromOptions(k)
        L.KSPSetInitialGuessNonzero(k, 1)
        V, val = C.c_void_p(), C.c_double()
        _set(L, u, uv); _set(L, b, bv)
        L.KSPSolve(k, b, u)
        x = sweeps(uv, bv, 3)
        r_old = bv - A @ x
        L.KSPBuildResidual(k, None, r, C.byref(V))
        L.VecNorm(V, NORM_2, C.byref(val))
        assert abs(val.value - np.linalg.norm(r_old)) <= 1e-12 * np.linalg.norm(r_old), case
        if case == "read r at once":
            assert np.max(np.abs(_get(L, r, n) - r_old)) <= rtol, case
        if case == "norm twice":
            L.VecNorm(V, NORM_2, C.byref(val))
            assert abs(val.value - np.linalg.norm(r_old)) <= 1e-12 * np.linalg.norm(r_old), case
        if case == "u written before the solve":
            L.VecScale(u, 0.5)
            x = 0.5 * x
        L.KSPSolve(k, b, u)                                  # adopts the three sweeps (except after the write to u)
        x3 = sweeps(x, bv, 3)
        if case == "reference order":
            L.KSPBuildResidual(k, None, r, C.byref(V))       # r overwritten unread (src/solver.c:1534)
            L.VecNorm(V, NORM_2, C.byref(val))
            assert abs(val.value - np.linalg.norm(bv - A @ x3)) <= 1e-11 * np.linalg.norm(bv - A @ x3), case
        elif case == "b rewritten after the solve":
            L.VecSet(b, 1.0)                                 # r was defined with the old b
            assert np.max(np.abs(_get(L, r, n) - r_old)) <= rtol, case
            assert np.all(_get(L, b, n) == 1.0)
        elif case == "second solve reuses the work vector":
            L.KSPSolve(k, b, u)                              # writes the work vector that holds the old iterate
            assert np.max(np.abs(_get(L, r, n) - r_old)) <= rtol, case
            x3 = sweeps(x3, bv, 3)
        elif case == "solver destroyed":
            L.KSPDestroy(C.byref(k))
            assert np.max(np.abs(_get(L, r, n) - r_old)) <= rtol, case
        elif case == "norm again after the solve":
            L.VecNorm(V, NORM_2, C.byref(val))
            assert abs(val.value - np.linalg.norm(r_old)) <= 1e-12 * np.linalg.norm(r_old), case
            assert np.max(np.abs(_get(L, r, n) - r_old)) <= rtol, case
        elif case == "restriction of r after the solve":
            Rm = _dense(orc, "R", npts, 0)
            mR = _assemble(L, Rm)
            bc = C.c_void_p()
            L.MatCreateVecs(mR, None, C.byref(bc))
            L.MatMult(mR, r, bc)
            assert np.max(np.abs(_get(L, bc, Rm.shape[0]) - Rm @ r_old)) <= rtol, case
            L.VecDestroy(C.byref(bc)); L.MatDestroy(C.byref(mR))
        elif case != "u written before the solve":
            assert np.max(np.abs(_get(L, r, n) - r_old)) <= rtol, case
        if case == "u written before the solve":
            assert np.max(np.abs(_get(L, r, n) - r_old)) <= rtol, case      # r belongs to u BEFORE the scaling
        assert np.max(np.abs(_get(L, u, n) - x3)) <= tol, case
        if k:
            L.KSPDestroy(C.byref(k))
        for v in (u, b, r):
            L.VecDestroy(C.byref(v))
    L.MatDestroy(C.byref(mA))


def recorded_coarse_subcycle_keeps_petsc_semantics(L, orc):
    """the drop-in RECORDS the reference's calls on the levels from 63^2 down and runs them as ONE tail launch when the pattern completes
    (DESIGN.md 8b N2, round 3).  Here the pattern is completed, interrupted, broken and abused in ways the reference never does; after every
    program each vector must hold what call-by-call execution gives (a numpy model runs the same program)."""
    L.PetscInitialize(None, None, None, None)
    L.PetscOptionsSetValue(None, b"-pc_type", b"jacobi")
    L.PetscOptionsSetValue(None, b"-ksp_richardson_scale", b"0.8")
    L.MatScale.argtypes = [C.c_void_p, C.c_double]
    npts, nlev = 33, 3
    A = [_dense(orc, "A", npts, l) for l in range(nlev)]
    R = [_dense(orc, "R", npts, l) for l in range(nlev - 1)]
    P = [_dense(orc, "P", npts, l) for l in range(nlev - 1)]
    rng = np.random.default_rng(23)
    b0v = rng.standard_normal(A[0].shape[0])

    programs = {
        "complete, then every intermediate read": ["cycle", "read_all"],
        "complete, b0 overwritten, then the intermediates read": ["cycle", ("set", "b0", 1.5), "read_all"],
        "complete, b0 scaled, then the intermediates read": ["cycle", ("scale", "b0", 2.0), "read_all"],
        "two cycles, the second overwrites the first's intermediates unread": ["cycle", ("scale", "b0", 0.5), "cycle", "read_all"],
        "b1 read in the middle of the descent": [("cycle", {"after_restrict0": [("read", "b1")]}), "read_all"],
        "u0 scaled in the middle of the descent": [("cycle", {"after_restrict0": [("scale", "u0", 2.0)]}), "read_all"],
        "u1 overwritten on the way up": [("cycle", {"after_prolong1": [("set", "u1", 0.25)]}), "read_all"],
        "another scale on level 1": [("cycle", {"before_solve1": [("kscale", 1, 0.5)]}), "read_all"],
        "two sweeps on level 0, three below": [("cycle", {"start": [("kits", 0, 2)]}), "read_all"],
        "A1 scaled in the middle of the ascent": [("cycle", {"after_prolong1": [("matscale", 1, 1.25)]}), "read_all", ("matscale", 1, 0.8)],
        "solver of level 1 destroyed after the cycle": ["cycle", ("kdestroy", 1), "read_all"],
        "descent abandoned after the first restriction": [("cycle", {"after_restrict0": ["stop"]}), "read_all"],
    }
    for name, prog in programs.items():
        mA, mR, mP = [_assemble(L, a) for a in A], [_assemble(L, r) for r in R], [_assemble(L, q) for q in P]
        V, M = {}, {}                                        # PETSc vectors / the numpy model's values
        for l in range(nlev):
            for nm in ("u", "b", "rv"):
                v = C.c_void_p()
                L.MatCreateVecs(mA[l], C.byref(v), None)
                V[nm + str(l)] = v
                M[nm + str(l)] = np.zeros(A[l].shape[0])
        _set(L, V["b0"], b0v); M["b0"] = b0v.copy()
        K, par = [], []
        for l in range(nlev):
            k = C.c_void_p()
            L.KSPCreate(1, C.byref(k))
            L.KSPSetType(k, b"richardson"); L.KSPSetOperators(k, mA[l], mA[l]); L.KSPSetNormType(k, 0)
            L.KSPSetTolerances(k, 1e-7, -2.0, -2.0, 3)
            L.KSPSetFromOptions(k)
            K.append(k); par.append({"its": 3, "scale": 0.8, "guess": 0, "A": A[l].copy(), "alive": True})

        def solve(l):
            x = M["u%d" % l] if par[l]["guess"] else np.zeros_like(M["u%d" % l])
            d = 1.0 / np.diag(par[l]["A"])
            for _ in range(par[l]["its"]):
                x = x + par[l]["scale"] * (d * (M["b%d" % l] - par[l]["A"] @ x))
            M["u%d" % l] = x
            L.KSPSolve(K[l], V["b%d" % l], V["u%d" % l])

        def extra(steps):
            for st in steps or []:
                if st == "stop":
                    return True
                if st[0] == "read":
                    assert np.max(np.abs(_get(L, V[st[1]], M[st[1]].size) - M[st[1]])) <= tol(st[1]), (name, st)
                elif st[0] == "scale":
                    L.VecScale(V[st[1]], st[2]); M[st[1]] = st[2] * M[st[1]]
                elif st[0] == "set":
                    L.VecSet(V[st[1]], st[2]); M[st[1]] = np.full_like(M[st[1]], st[2])
                elif st[0] == "kscale":
                    L.KSPRichardsonSetScale(K[st[1]], st[2]); par[st[1]]["scale"] = st[2]
                elif st[0] == "kits":
                    L.KSPSetTolerances(K[st[1]], 1e-7, -2.0, -2.0, st[2]); par[st[1]]["its"] = st[2]
                elif st[0] == "matscale":
                    L.MatScale(mA[st[1]], st[2]); par[st[1]]["A"] = st[2] * par[st[1]]["A"]
                elif st[0] == "kdestroy":
                    L.KSPDestroy(C.byref(K[st[1]])); par[st[1]]["alive"] = False
            return False

        def tol(nm):
            return 1e-11 * max(1.0, np.abs(M[nm]).max())

        def cycle(hooks):
            # the reference's loop on these levels (src/solver.c:1531-1544), every solver back to the zero guess first
            for l in range(nlev):
                L.KSPSetInitialGuessNonzero(K[l], 0); par[l]["guess"] = 0
            if extra(hooks.get("start")):
                return
            solve(0)
            L.KSPSetInitialGuessNonzero(K[0], 1); par[0]["guess"] = 1
            for l in range(1, nlev):
                Vp = C.c_void_p()
                L.KSPBuildResidual(K[l - 1], None, V["rv%d" % (l - 1)], C.byref(Vp))
                M["rv%d" % (l - 1)] = M["b%d" % (l - 1)] - par[l - 1]["A"] @ M["u%d" % (l - 1)]
                L.MatMult(mR[l - 1], Vp, V["b%d" % l])
                M["b%d" % l] = R[l - 1] @ M["rv%d" % (l - 1)]
                if extra(hooks.get("after_restrict%d" % (l - 1))):
                    return
                if extra(hooks.get("before_solve%d" % l)):
                    return
                solve(l)
                if l != nlev - 1:
                    L.KSPSetInitialGuessNonzero(K[l], 1); par[l]["guess"] = 1
            for l in range(nlev - 2, -1, -1):
                L.MatMult(mP[l], V["u%d" % (l + 1)], V["rv%d" % l])
                M["rv%d" % l] = P[l] @ M["u%d" % (l + 1)]
                if extra(hooks.get("after_prolong%d" % l)):
                    return
                L.VecAXPY(V["u%d" % l], 1.0, V["rv%d" % l])
                M["u%d" % l] = M["u%d" % l] + M["rv%d" % l]
                solve(l)
                if l != 0:
                    L.KSPSetInitialGuessNonzero(K[l], 0); par[l]["guess"] = 0

        for st in prog:
            if st == "cycle":
                cycle({})
            elif st == "read_all":
                for nm in sorted(M):
                    assert np.max(np.abs(_get(L, V[nm], M[nm].size) - M[nm])) <= tol(nm), (name, nm)
            elif st[0] == "cycle":
                cycle(st[1])
            else:
                extra([st])
        for l in range(nlev):
            if par[l]["alive"]:
                L.KSPDestroy(C.byref(K[l]))
        for v in V.values():
            L.VecDestroy(C.byref(v))
        for m in mA + mR + mP:
            L.MatDestroy(C.byref(m))


def deferred_values_around_the_recorder(L, orc):
    """two call orders the extended random programs found (both gave O(1) errors in the default mode, none with MGPETSC_TAIL=0), pinned:
    1. a recording is open and has taken the restricted right-hand side b2; the solver of level 2 is Chebyshev, which the recorder is not
       asked about.  Its KSPSolve makes b2 concrete: the recording is replayed call by call, and the replayed MatMult(res) defers b2 again
       (R (b1 - A1 u1)) -- the solve read b2's buffer before the restriction had run.
    2. a sub-cycle has run as ONE tail launch with b1 as its right-hand side; rv0 = P b1 is deferred (MatMult(pro)); b1 is overwritten
       entirely.  The finished log takes b1's buffer and b1 continues on a spare one -- from which the deferred P b1 was then formed."""
    from cheby_reference import cheb_steps
    L.PetscInitialize(None, None, None, None)
    L.PetscOptionsSetValue(None, b"-pc_type", b"jacobi")
    L.KSPChebyshevSetEigenvalues.argtypes = [C.c_void_p, C.c_double, C.c_double]
    npts = 33
    A = [_dense(orc, "A", npts, l) for l in range(3)]
    R = [_dense(orc, "R", npts, l) for l in range(2)]
    P = [_dense(orc, "P", npts, l) for l in range(2)]
    mA, mR, mP = [_assemble(L, a) for a in A], [_assemble(L, r) for r in R], [_assemble(L, q) for q in P]
    d = [1.0 / np.diag(a) for a in A]
    rng = np.random.default_rng(43)
    b1v = rng.standard_normal(A[1].shape[0])

    def vec(l):
        v = C.c_void_p()
        L.MatCreateVecs(mA[l], C.byref(v), None)
        return v

    def solver(l, cheby, maxit):
        k = C.c_void_p()
        L.KSPCreate(1, C.byref(k))
        L.KSPSetType(k, b"chebyshev" if cheby else b"richardson"); L.KSPSetOperators(k, mA[l], mA[l]); L.KSPSetNormType(k, 0)
        L.KSPSetTolerances(k, 1e-7, -2.0, -2.0, maxit)
        L.KSPSetFromOptions(k)
        L.KSPRichardsonSetScale(k, 0.8)
        if cheby:
            L.KSPChebyshevSetEigenvalues(k, 2.0, 0.2)
        return k

    def sweeps(l, x, rhs, m):
        for _ in range(m):
            x = x + 0.8 * (d[l] * (rhs - A[l] @ x))
        return x

    def close(v, want, what):
        err = float(np.max(np.abs(_get(L, v, want.size) - want)))
        assert err <= 1e-11 * max(1.0, float(np.abs(want).max())), (what, err)

    V = C.c_void_p()
    for cheby in (True, False):
        rv0, b1, u1, r1, b2, u2 = vec(0), vec(1), vec(1), vec(1), vec(2), vec(2)
        k1, k2 = solver(1, False, 2), solver(2, cheby, 3)
        _set(L, b1, b1v)
        L.KSPSolve(k1, b1, u1)                               # zero guess, 15^2: a recording starts
        L.KSPSetInitialGuessNonzero(k1, 1)
        L.KSPBuildResidual(k1, None, r1, C.byref(V))
        L.MatMult(mR[1], V, b2)
        L.KSPSolve(k2, b2, u2)                               # Chebyshev: interrupts the recording; Richardson: continues it
        m_u1 = sweeps(1, np.zeros_like(b1v), b1v, 2)
        m_b2 = R[1] @ (b1v - A[1] @ m_u1)
        if cheby:
            s, cs = cheb_steps(0.2, 2.0, 3)
            pkm1, pk = np.zeros_like(m_b2), s * (d[2] * m_b2)
            for a, w, g in cs:
                pkm1, pk = pk, (a * pkm1 + w * pk) + g * (d[2] * (m_b2 - A[2] @ pk))
            m_u2 = pk
            close(u2, m_u2, "1: Chebyshev solve on the right-hand side an open recording had taken")
            close(b2, m_b2, "1: that right-hand side")
        else:
            m_u2 = sweeps(2, np.zeros_like(m_b2), m_b2, 3)
        L.MatMult(mP[1], u2, r1)
        L.VecAXPY(u1, 1.0, r1)
        L.KSPSolve(k1, b1, u1)                               # Richardson below: the pattern is complete, ONE tail launch
        m_u1 = sweeps(1, m_u1 + P[1] @ m_u2, b1v, 2)
        L.MatMult(mP[0], b1, rv0)                            # rv0 = P b1, deferred
        L.VecSet(b1, 1.0)                                    # the finished log keeps the old b1
        close(rv0, P[0] @ b1v, "2: P b1 deferred, then b1 overwritten while a finished log names it")
        close(u1, m_u1, "2: u1")
        close(u2, m_u2, "2: u2 (an unread intermediate of the tail launch)")
        close(b2, m_b2, "2: b2 (likewise)")
        assert np.all(_get(L, b1, b1v.size) == 1.0)
        L.KSPDestroy(C.byref(k1)); L.KSPDestroy(C.byref(k2))
        for v in (rv0, b1, u1, r1, b2, u2):
            L.VecDestroy(C.byref(v))
    for m in mA + mR + mP:
        L.MatDestroy(C.byref(m))


def pcmg_level_vectors_after_the_tail_launch(L, orc):
    """-cycle 8 set up as the reference does (src/solver.c:1918-1956: its own vectors handed to PCMG through PCMGSetRhs / PCMGSetX / PCMGSetR), full
    depth, PETSc's default exact coarse solve: the drop-in runs PCMG's levels from 63^2 down -- here all of them -- as ONE tail launch and does
    not compute the level vectors.  Reading them after the solve must give what the level-by-level cycle leaves there (numpy model)."""
    L.PetscInitialize(None, None, None, None)
    for k_, v_ in ((b"-mg_levels_ksp_type", b"richardson"), (b"-mg_levels_pc_type", b"jacobi"), (b"-mg_levels_ksp_max_it", b"3"),
                   (b"-mg_levels_ksp_richardson_scale", b"0.8")):
        L.PetscOptionsSetValue(None, k_, v_)
    npts, nlev = 33, 5
    A = [_dense(orc, "A", npts, l) for l in range(nlev)]
    R = [_dense(orc, "R", npts, l) for l in range(nlev - 1)]
    P = [_dense(orc, "P", npts, l) for l in range(nlev - 1)]
    mA, mR, mP = [_assemble(L, a) for a in A], [_assemble(L, r) for r in R], [_assemble(L, q) for q in P]
    rng = np.random.default_rng(31)
    b0v = rng.standard_normal(A[0].shape[0])
    u, b, r = [], [], []
    for l in range(nlev):
        for lst in (u, b, r):
            v = C.c_void_p()
            L.MatCreateVecs(mA[l], C.byref(v), None)
            lst.append(v)
    _set(L, b[0], b0v)
    ksp, pc, kt = C.c_void_p(), C.c_void_p(), C.c_void_p()
    L.KSPCreate(1, C.byref(ksp))
    L.KSPSetType(ksp, b"richardson"); L.KSPSetOperators(ksp, mA[0], mA[0]); L.KSPSetNormType(ksp, 2)
    L.KSPSetTolerances(ksp, 1e-30, -2.0, -2.0, 2)                       # two applications of the preconditioner
    L.KSPGetPC(ksp, C.byref(pc))
    L.PCSetType(pc, b"mg")
    L.PCMGSetLevels(pc, nlev, None)
    L.PCMGGetCoarseSolve(pc, C.byref(kt)); L.KSPSetOperators(kt, mA[nlev - 1], mA[nlev - 1])
    for i in range(1, nlev):
        L.PCMGGetSmoother(pc, i, C.byref(kt)); L.KSPSetOperators(kt, mA[nlev - i - 1], mA[nlev - i - 1])
        L.PCMGSetInterpolation(pc, i, mP[nlev - i - 1]); L.PCMGSetRestriction(pc, i, mR[nlev - i - 1])
    L.PCMGSetR(pc, nlev - 1, r[0])
    for i in range(1, nlev - 1):
        L.PCMGSetRhs(pc, i, b[nlev - i - 1]); L.PCMGSetX(pc, i, u[nlev - i - 1]); L.PCMGSetR(pc, i, r[nlev - i - 1])
    L.PCMGSetRhs(pc, 0, b[nlev - 1]); L.PCMGSetX(pc, 0, u[nlev - 1])
    L.KSPSetFromOptions(ksp)
    L.KSPSolve(ksp, b[0], u[0])
    # the numpy model: outer Richardson (scale 1), PCMG V-cycle with 3 + 3 damped Jacobi sweeps, exact solve on the 1 x 1 grid
    lev = {}

    def sm(l, x, rhs, m):
        d = 1.0 / np.diag(A[l])
        for _ in range(m):
            x = x + 0.8 * (d * (rhs - A[l] @ x))
        return x

    def cyc(l, rhs):
        if l == nlev - 1:
            x = np.linalg.solve(A[l], rhs)
        else:
            x = sm(l, np.zeros_like(rhs), rhs, 3)
            bc = R[l] @ (rhs - A[l] @ x)
            x = x + P[l] @ cyc(l + 1, bc)
            x = sm(l, x, rhs, 3)
        if l > 0:
            lev[l] = (rhs.copy(), x.copy())
        return x

    x = np.zeros_like(b0v)
    for _ in range(2):
        x = x + cyc(0, b0v - A[0] @ x)
    tol = 1e-11 * max(1.0, np.abs(x).max())
    assert np.max(np.abs(_get(L, u[0], x.size) - x)) <= tol
    for l in range(nlev - 1, 0, -1):                                     # the level vectors, coarsest first, then once more in the other order
        assert np.max(np.abs(_get(L, u[l], lev[l][1].size) - lev[l][1])) <= 1e-11 * max(1.0, np.abs(lev[l][1]).max()), ("u", l)
        assert np.max(np.abs(_get(L, b[l], lev[l][0].size) - lev[l][0])) <= 1e-11 * max(1.0, np.abs(lev[l][0]).max()), ("b", l)
    for l in range(1, nlev):
        assert np.max(np.abs(_get(L, u[l], lev[l][1].size) - lev[l][1])) <= 1e-11 * max(1.0, np.abs(lev[l][1]).max()), ("u again", l)
    L.KSPDestroy(C.byref(ksp))
    for v in u + b + r:
        L.VecDestroy(C.byref(v))
    for m in mA + mR + mP:
        L.MatDestroy(C.byref(m))


def richardson_with_lu_is_damped_not_exact(L, orc):
    """-pc_type lu (the dense inverse of a small operator): preonly and richardson with scale 1 return A^-1 b whatever the guess;
    richardson with scale s != 1 makes max_it DAMPED steps x <- (1 - s) x + s A^-1 b, as PETSc would (it used to come
    back as the exact solution, silently)."""
    L.PetscInitialize(None, None, None, None)
    L.PetscOptionsSetValue(None, b"-pc_type", b"lu")
    A = _dense(orc, "A", 17, 0)
    mA = _assemble(L, A)
    n = A.shape[0]
    rng = np.random.default_rng(5)
    bv, x0 = rng.standard_normal(n), rng.standard_normal(n)
    y = np.linalg.solve(A, bv)
    u, b = C.c_void_p(), C.c_void_p()
    L.MatCreateVecs(mA, C.byref(u), C.byref(b))
    _set(L, b, bv)
    tol = 1e-10 * np.abs(y).max()
    for ktype, scale, maxit, guess in ((b"preonly", 1.0, 1, 0), (b"richardson", 1.0, 2, 1), (b"richardson", 1.0, 1, 0),
                                       (b"richardson", 0.5, 3, 0), (b"richardson", 0.5, 3, 1), (b"richardson", 1.3, 2, 1), (b"richardson", 0.7, 0, 1)):
        k = C.c_void_p()
        L.KSPCreate(1, C.byref(k))
        L.KSPSetType(k, ktype); L.KSPSetOperators(k, mA, mA); L.KSPSetNormType(k, 0)
        L.KSPSetTolerances(k, 1e-7, -2.0, -2.0, maxit)
        L.KSPSetFromOptions(k)
        L.KSPRichardsonSetScale(k, scale)
        L.KSPSetInitialGuessNonzero(k, guess)
        _set(L, u, x0)
        L.KSPSolve(k, b, u)
        x = x0.copy() if guess else np.zeros(n)
        if ktype == b"preonly":
            x = y
        else:
            for _ in range(maxit):
                x = (1.0 - scale) * x + scale * y
        got = _get(L, u, n)
        assert np.max(np.abs(got - x)) <= tol, (ktype, scale, maxit, guess, np.max(np.abs(got - x)))
        L.KSPDestroy(C.byref(k))
    for v in (u, b):
        L.VecDestroy(C.byref(v))
    L.MatDestroy(C.byref(mA))


MODES = {      # the drop-in's environment switches, each read once per process: one child process per mode
    "eager": {"MGPETSC_LAZY": "0"},
    "notail": {"MGPETSC_TAIL": "0"},
    "lazy2": {"MGPETSC_LAZY": "2"},
    "noj3": {"MGPETSC_J3": "0"},
    "keepr0": {"MGPETSC_KEEP_R": "0"},
    "round2": {"MGPETSC_J3": "0", "MGPETSC_TAIL": "0"},
    "pairs": {"MGPETSC_PAIR_MIN_N": "7"},
    "pairs_noj3": {"MGPETSC_PAIR_MIN_N": "7", "MGPETSC_J3": "0"},
    "generic": {"MGPETSC_NO_RECOGNITION": "1"},
}
LAZY_STATS_RE = (r"lazy temporaries: (\d+) residual\+restriction passes, (\d+) prolongation sweeps fused; computed after all: (\d+) residuals, "
                 r"(\d+) prolongations, (\d+) corrections; (\d+) dropped unread; (\d+) zero-guess sweeps out of the restriction's pass; "
                 r"(\d+) norm passes that store r and make the next sweep, (\d+) of those sweeps adopted; "
                 r"(\d+) norm passes that left r deferred, (\d+) of those residuals followed the old iterate into the work vector; "
                 r"(\d+) coarse sub-cycles run as ONE tail launch, (\d+) recordings replayed call by call, (\d+) times their unread intermediates "
                 r"were computed after all; (\d+) three-sweep passes, (\d+) two-sweep passes of KSPSolve")


def lazy_stats(out):
    """the sixteen counters PetscFinalize prints under MGPETSC_LAZY_STATS=1, in the order of the line: eleven of the lazy temporaries, three of
    the tail recorder, three-sweep passes, two-sweep passes of KSPSolve"""
    import re
    m = re.search(LAZY_STATS_RE, out)
    assert m, out[-1500:]
    return [int(x) for x in m.groups()]


def random_programs_went_the_way_of_the_mode(mode, st):
    """st: lazy_stats() of a child that ran the extended random programs under MODES[mode] (None: no switch set).  A mode that silently ran the
    default paths would pass every comparison with the model: the counters show that the switch switched, and that the default draw does
    reach the recorder, the three-sweep passes and the norm pass that leaves r deferred.  (Every level is at most 63 wide: below the
    default pairing threshold, inside the recorder's range.)"""
    lazy, tail, three, two = st[:11], st[11:14], st[14], st[15]
    if mode in ("eager", "generic"):                 # nothing deferred / no recognised operator to defer on
        assert lazy == [0] * 11, (mode, st)
    else:
        assert lazy[0] > 0 and lazy[1] > 0, (mode, st)
    if mode in ("eager", "notail", "round2", "lazy2", "generic"):      # (the recorder needs MGPETSC_LAZY=1)
        assert tail == [0, 0, 0], (mode, st)
    else:
        assert tail[0] > 0 and tail[1] > 0, (mode, st)                 # logs that ran as one launch, and logs that were interrupted
    assert (three == 0) == (mode in ("noj3", "round2", "pairs_noj3", "generic")), (mode, st)
    assert (two > 0) == (mode in ("pairs", "pairs_noj3")), (mode, st)
    if mode in ("keepr0", "lazy2", "noj3", "round2", "pairs_noj3"):    # r is left deferred only by the three-sweep norm pass, only under MGPETSC_LAZY=1
        assert lazy[9] == 0, (mode, st)
    if mode in (None, "notail", "pairs"):
        assert lazy[9] > 0, (mode, st)
    if mode == "lazy2":                              # b_c is not deferred: no coarse sweep out of the restriction's pass, no norm pass with a sweep
        assert lazy[6] == 0 and lazy[7] == 0, (mode, st)


def random_programs_keep_petsc_semantics(L, orc, seed=1, nprog=40, nops=60, extended=False):
    """Programs of PETSc calls drawn at random over a two-level set-up (fine / coarse 5-point operators, full weighting, bilinear prolongation,
    two Richardson + Jacobi solvers, six fine and three coarse vectors) against a numpy model that executes call by call: residuals, transfers,
    corrections, BLAS-1, norms, solves with changing max_it / scale / guess flag, reads, destroy + re-create -- with the fragments of the
    reference's loop (src/solver.c:1531-1546) among the draws, so that the drop-in's deferred temporaries, speculative sweeps and fused passes
    start and are then interrupted wherever the draw says.  Every value read, every norm and every vector at the end of a program must be what
    call-by-call execution gives (tolerance: 1e-11 of a running magnitude bound of the vector; the arithmetic order differs from numpy's).

    extended: each program also draws its depth (2 or 3 levels, three more vectors on the third; transfers, frag_down and frag_up act between
    an adjacent pair, frag_cycle is the whole cycle of that depth -- half of the time with the solvers brought to one damping factor and one
    sweep count and the guess flags set as the reference sets them, so that the recorder's pattern completes), its operator (the uniform
    stencil, or a row table with W != E on every level: tests/coef_cases.py) and the type of each solver (Richardson, or Chebyshev with
    eigenvalue bounds drawn once per solver; model: the restarted recurrence of tests/cheby_reference.py, whose first step is taken at
    max_it = 0 too; its magnitude bound grows by |c_km1| + |c_k| and |c_z| per step).  With MGPETSC_NO_RECOGNITION set every solver is
    Richardson: the drop-in refuses Chebyshev on an assembled AIJ operator.  Not extended: the draw is call for call what it was.
    Returns the largest error-to-bound ratio met (1.0 is the tolerance)."""
    import os
    from cheby_reference import EIGS, cheb_steps
    from coef_cases import distinct_row_tables
    L.PetscInitialize(None, None, None, None)
    L.PetscOptionsSetValue(None, b"-pc_type", b"jacobi")
    L.KSPChebyshevSetEigenvalues.argtypes = [C.c_void_p, C.c_double, C.c_double]
    rng = np.random.default_rng(seed)
    no_cheby = bool(os.environ.get("MGPETSC_NO_RECOGNITION"))
    worst = [0.0]
    for prog in range(nprog):
        npts = int(rng.choice([17, 33, 33, 65]))
        depth, rows = 2, False
        if extended:
            depth, rows = int(rng.integers(2, 4)), bool(rng.integers(0, 2))
        Rl = [_dense(orc, "R", npts, l) for l in range(depth - 1)]
        Pl = [_dense(orc, "P", npts, l) for l in range(depth - 1)]
        if rows:
            width = [(npts - 1) // 2 ** l - 1 for l in range(depth)]
            Al = [_five_point(n_, (lambda ct: lambda i: ct[i])(distinct_row_tables(rng, n_)[0])) for n_ in width]
        else:
            Al = [_dense(orc, "A", npts, l) for l in range(depth)]
        mAl, mPl, mRl = [_assemble(L, a) for a in Al], [_assemble(L, p_) for p_ in Pl], [_assemble(L, r_) for r_ in Rl]
        size = [a.shape[0] for a in Al]
        amax = {l: 5.0 * np.abs(Al[l]).max() for l in range(depth)}
        dinv = {l: 1.0 / np.diag(Al[l]) for l in range(depth)}
        dmax = {l: float(np.abs(dinv[l]).max()) if rows else float(dinv[l].max()) for l in range(depth)}
        Aop = dict(enumerate(Al))
        pools = [["x", "b", "r", "rv", "u", "w"], ["uc", "bc", "rc"], ["ud", "bd", "rd"]][:depth]
        allv = [v for pool in pools for v in pool]
        lev = {v: l for l, pool in enumerate(pools) for v in pool}
        H, M, mag = {}, {}, {}
        first = [C.c_void_p() for _ in range(depth)]
        for l in range(depth):
            L.MatCreateVecs(mAl[l], C.byref(first[l]), None)
        for v in allv:
            h = C.c_void_p()
            L.VecDuplicate(first[lev[v]], C.byref(h))
            H[v] = h
            M[v] = rng.standard_normal(size[lev[v]])
            mag[v] = float(np.abs(M[v]).max())
            _set(L, h, M[v])
        K, kst = {}, {}
        for q in range(depth):
            k = C.c_void_p()
            L.KSPCreate(1, C.byref(k))
            kst[q] = {"maxit": int(rng.integers(0, 5)), "scale": float(rng.choice([0.5, 0.8, 1.0])), "guess": int(rng.integers(0, 2)), "b": None, "x": None,
                      "cheby": None}
            if extended and not no_cheby and rng.integers(0, 2):
                kst[q]["cheby"] = EIGS[int(rng.integers(0, len(EIGS)))]
            L.KSPSetType(k, b"chebyshev" if kst[q]["cheby"] else b"richardson"); L.KSPSetOperators(k, mAl[q], mAl[q]); L.KSPSetNormType(k, 0)
            L.KSPSetTolerances(k, 1e-7, -2.0, -2.0, kst[q]["maxit"])
            L.KSPSetFromOptions(k)
            L.KSPRichardsonSetScale(k, kst[q]["scale"])
            if kst[q]["cheby"]:
                L.KSPChebyshevSetEigenvalues(k, kst[q]["cheby"][1], kst[q]["cheby"][0])
            L.KSPSetInitialGuessNonzero(k, kst[q]["guess"])
            K[q] = k
        trace = []

        def pick(level, n=1, exclude=()):
            pool = [v for v in pools[level] if v not in exclude]
            return [str(t) for t in rng.choice(pool, size=n, replace=False)]

        def pair():                              # the finer level of an adjacent pair
            return int(rng.integers(0, depth - 1)) if depth > 2 else 0

        def check(v, what):
            got = _get(L, H[v], size[lev[v]])
            err = float(np.max(np.abs(got - M[v])))
            worst[0] = max(worst[0], err / (1e-11 * max(mag[v], 1e-30) + 1e-300))
            assert err <= 1e-11 * max(mag[v], 1e-30) + 1e-300, (f"seed {seed} program {prog}: {what} of {v}: error {err:.3e} against magnitude {mag[v]:.3e}", trace)

        def check_norm(v, what):
            val = C.c_double()
            L.VecNorm(H[v], NORM_2, C.byref(val))
            bound = 1e-11 * np.sqrt(M[v].size) * max(mag[v], 1e-30) + 1e-300
            worst[0] = max(worst[0], abs(val.value - np.linalg.norm(M[v])) / bound)
            assert abs(val.value - np.linalg.norm(M[v])) <= bound, (f"seed {seed} program {prog}: {what}: {val.value!r} against {np.linalg.norm(M[v])!r}", trace)

        def residual(q, bn, xn, rn_, via_ksp):
            if via_ksp:
                V = C.c_void_p()
                L.KSPBuildResidual(K[q], None, H[rn_], C.byref(V))
            else:
                L.MatResidual(mAl[q], H[bn], H[xn], H[rn_])
            M[rn_] = M[bn] - Aop[q] @ M[xn]
            mag[rn_] = mag[bn] + amax[q] * mag[xn]

        def restrict(l, f, c):
            L.MatMult(mRl[l], H[f], H[c]); M[c] = Rl[l] @ M[f]; mag[c] = mag[f]

        def prolong(l, c, f):
            L.MatMult(mPl[l], H[c], H[f]); M[f] = Pl[l] @ M[c]; mag[f] = mag[c]

        def correct(u_, rv_):
            L.VecAXPY(H[u_], 1.0, H[rv_]); M[u_] = M[u_] + M[rv_]; mag[u_] = mag[u_] + mag[rv_]

        def solve(q, bn, xn):
            st = kst[q]
            L.KSPSolve(K[q], H[bn], H[xn])
            xm = M[xn].copy() if st["guess"] else np.zeros_like(M[xn])
            mg = mag[xn] if st["guess"] else 0.0
            if st["cheby"]:
                s, cs = cheb_steps(st["cheby"][0], st["cheby"][1], max(st["maxit"], 1))
                pkm1, mkm1 = xm, mg
                pk = pkm1 + s * (dinv[q] * (M[bn] - Aop[q] @ pkm1))
                mk = mkm1 + s * dmax[q] * (mag[bn] + amax[q] * mkm1)
                for c_km1, c_k, c_z in cs:
                    z = dinv[q] * (M[bn] - Aop[q] @ pk)
                    pkm1, pk = pk, (c_km1 * pkm1 + c_k * pk) + c_z * z
                    mkm1, mk = mk, abs(c_km1) * mkm1 + abs(c_k) * mk + abs(c_z) * dmax[q] * (mag[bn] + amax[q] * mk)
                xm, mg = pk, mk
            else:
                for _ in range(st["maxit"]):
                    xm = xm + st["scale"] * (dinv[q] * (M[bn] - Aop[q] @ xm))
                    mg = mg + st["scale"] * dmax[q] * (mag[bn] + amax[q] * mg)
            M[xn], mag[xn] = xm, max(mg, float(np.abs(xm).max()))
            st["b"], st["x"] = bn, xn

        def param(q, what, value):
            kst[q][what] = value
            if what == "maxit":
                L.KSPSetTolerances(K[q], 1e-7, -2.0, -2.0, value)
            elif what == "scale":
                L.KSPRichardsonSetScale(K[q], value)
            else:
                L.KSPSetInitialGuessNonzero(K[q], value)

        for step in range(nops):
            op = str(rng.choice(["resid", "kresid", "restrict", "prolong", "apply", "axpy", "scale", "set", "copy", "norm", "solve", "solve", "param", "read",
                                 "recreate", "frag_down", "frag_up", "frag_up", "frag_norm", "frag_norm", "frag_cycle"]))
            q = int(rng.integers(0, depth))
            if op == "resid":
                bn, xn, rn_ = pick(q, 3)
                trace.append(f"MatResidual(A{q}, {bn}, {xn}, {rn_})")
                residual(q, bn, xn, rn_, False)
            elif op == "kresid":
                if kst[q]["b"] is None:
                    continue
                (rn_,) = pick(q, 1, exclude=(kst[q]["b"], kst[q]["x"]))
                trace.append(f"KSPBuildResidual(k{q}, {rn_})   [b={kst[q]['b']}, x={kst[q]['x']}]")
                residual(q, kst[q]["b"], kst[q]["x"], rn_, True)
            elif op == "restrict":
                l = pair()
                (f,), (c,) = pick(l), pick(l + 1)
                trace.append(f"MatMult(R{l}, {f}, {c})")
                restrict(l, f, c)
            elif op == "prolong":
                l = pair()
                (f,), (c,) = pick(l), pick(l + 1)
                trace.append(f"MatMult(P{l}, {c}, {f})")
                prolong(l, c, f)
            elif op == "apply":
                a, bb = pick(q, 2)
                trace.append(f"MatMult(A{q}, {a}, {bb})")
                L.MatMult(mAl[q], H[a], H[bb]); M[bb] = Aop[q] @ M[a]; mag[bb] = amax[q] * mag[a]
            elif op == "axpy":
                y, xx = pick(q, 2)
                al = float(rng.choice([1.0, -1.0, 0.5, 2.0]))
                trace.append(f"VecAXPY({y}, {al}, {xx})")
                L.VecAXPY(H[y], al, H[xx]); M[y] = M[y] + al * M[xx]; mag[y] = mag[y] + abs(al) * mag[xx]
            elif op == "scale":
                (v,) = pick(q)
                al = float(rng.choice([0.5, -1.0, 2.0, 0.0]))
                trace.append(f"VecScale({v}, {al})")
                L.VecScale(H[v], al); M[v] = al * M[v]; mag[v] = abs(al) * mag[v]
            elif op == "set":
                (v,) = pick(q)
                al = float(rng.choice([0.0, 1.0, -2.5]))
                trace.append(f"VecSet({v}, {al})")
                L.VecSet(H[v], al); M[v] = np.full_like(M[v], al); mag[v] = abs(al)
            elif op == "copy":
                a, bb = pick(q, 2)
                trace.append(f"VecCopy({a}, {bb})")
                L.VecCopy(H[a], H[bb]); M[bb] = M[a].copy(); mag[bb] = mag[a]
            elif op == "norm":
                (v,) = pick(q)
                trace.append(f"VecNorm({v})")
                check_norm(v, f"norm of {v}")
            elif op == "solve":
                bn, xn = pick(q, 2)
                trace.append(f"KSPSolve(k{q}, {bn}, {xn})   [max_it={kst[q]['maxit']} scale={kst[q]['scale']} guess={kst[q]['guess']} cheby={kst[q]['cheby']}]")
                solve(q, bn, xn)
            elif op == "param":
                what = str(rng.choice(["maxit", "scale", "guess"]))
                if what == "maxit":
                    param(q, "maxit", int(rng.integers(0, 5)))
                elif what == "scale":
                    param(q, "scale", float(rng.choice([0.5, 0.8, 1.0])))
                else:
                    param(q, "guess", int(rng.integers(0, 2)))
                trace.append(f"k{q}.{what} = {kst[q][what]}")
            elif op == "read":
                (v,) = pick(q)
                trace.append(f"read {v}")
                check(v, "read")
            elif op == "recreate":
                (v,) = pick(q, 1, exclude=(kst[q]["b"], kst[q]["x"]))       # (the solver's vectors stay: KSPBuildResidual refers to them)
                trace.append(f"VecDestroy({v}); VecDuplicate; VecSet(1.5)")
                L.VecDestroy(C.byref(H[v]))
                h = C.c_void_p()
                L.VecDuplicate(first[q], C.byref(h))
                H[v] = h
                L.VecSet(h, 1.5); M[v] = np.full_like(M[v], 1.5); mag[v] = 1.5
            elif op == "frag_down":          # src/solver.c:1534-1536
                l = pair()
                if kst[l]["b"] is None:
                    continue
                (rn_,) = pick(l, 1, exclude=(kst[l]["b"], kst[l]["x"]))
                bc_, uc_ = pick(l + 1, 2)
                trace.append(f"down: KSPBuildResidual(k{l}, {rn_}); MatMult(R{l}, {rn_}, {bc_}); KSPSolve(k{l + 1}, {bc_}, {uc_})")
                residual(l, kst[l]["b"], kst[l]["x"], rn_, True)
                restrict(l, rn_, bc_)
                solve(l + 1, bc_, uc_)
            elif op == "frag_up":            # :1540-1542
                l = pair()
                (uc_,) = pick(l + 1)
                rv_, u_, b_ = pick(l, 3)
                if kst[l]["x"] is not None and rng.integers(0, 2):
                    u_, b_ = kst[l]["x"], kst[l]["b"]
                    if rv_ in (u_, b_):
                        (rv_,) = pick(l, 1, exclude=(u_, b_))
                trace.append(f"up: MatMult(P{l}, {uc_}, {rv_}); VecAXPY({u_}, 1, {rv_}); KSPSolve(k{l}, {b_}, {u_})")
                prolong(l, uc_, rv_)
                correct(u_, rv_)
                solve(l, b_, u_)
            elif op == "frag_norm":          # :1545-1546 and the next :1531
                l = int(rng.integers(0, depth)) if extended else 0
                if kst[l]["b"] is None:
                    continue
                (rn_,) = pick(l, 1, exclude=(kst[l]["b"], kst[l]["x"]))
                trace.append(f"norm: KSPBuildResidual(k{l}, {rn_}); VecNorm({rn_})" + (f"; KSPSolve(k{l}, same b, same x)" if step % 2 else ""))
                residual(l, kst[l]["b"], kst[l]["x"], rn_, True)
                check_norm(rn_, "residual norm")
                if step % 2:
                    solve(l, kst[l]["b"], kst[l]["x"])
            elif op == "frag_cycle":         # one whole cycle of the reference's loop over every level of the program, on fixed vectors
                U, B, RES, COR = ["u", "uc", "ud"], ["b", "bc", "bd"], ["r", "rc"], ["rv", "rc"]     # (below level 0 r and rv are one vector, as in the reference)
                ref_flags = bool(extended and rng.integers(0, 2))
                trace.append(f"cycle over {depth} levels: KSPSolve(k0,b,u); down {{KSPBuildResidual; MatMult(R); KSPSolve}}; up {{MatMult(P); VecAXPY; KSPSolve}}; "
                             "KSPBuildResidual(k0,r); VecNorm(r)" + (" -- one scale, one max_it, the guess flags of src/solver.c:1532-1543" if ref_flags else ""))
                if ref_flags:
                    sc, v0 = float(rng.choice([0.5, 0.8, 1.0])), int(rng.integers(1, 5))
                    for l in range(depth):
                        param(l, "scale", sc)
                        param(l, "maxit", v0 if l < depth - 1 else int(rng.integers(1, 5)))
                        param(l, "guess", int(rng.integers(0, 2)) if l == 0 else 0)
                trace.append("   with " + "; ".join(f"k{l}: max_it={kst[l]['maxit']} scale={kst[l]['scale']} guess={kst[l]['guess']} cheby={kst[l]['cheby']}" for l in range(depth)))
                solve(0, "b", "u")
                if ref_flags:
                    param(0, "guess", 1)
                for l in range(1, depth):
                    residual(l - 1, B[l - 1], U[l - 1], RES[l - 1], True)
                    restrict(l - 1, RES[l - 1], B[l])
                    solve(l, B[l], U[l])
                    if ref_flags and l != depth - 1:
                        param(l, "guess", 1)
                for l in range(depth - 2, -1, -1):
                    prolong(l, U[l + 1], COR[l])
                    correct(U[l], COR[l])
                    solve(l, B[l], U[l])
                    if ref_flags and l != 0:
                        param(l, "guess", 0)
                residual(0, "b", "u", "r", True)
                check_norm("r", "cycle norm")
            if max(mag.values()) > 1e200:        # (a draw that keeps multiplying by A: start the next program)
                break
        for v in allv:
            check(v, "final value")
        for q in range(depth):
            L.KSPDestroy(C.byref(K[q]))
        for v in allv:
            L.VecDestroy(C.byref(H[v]))
        for h in first:
            L.VecDestroy(C.byref(h))
        for m in mAl + mPl + mRl:
            L.MatDestroy(C.byref(m))
    print(f"random programs (seed {seed}, {nprog} programs{', extended draw' if extended else ''}): largest error / bound = {worst[0]:.3e}")
    if os.environ.get("MGPETSC_LAZY_STATS"):       # which of the drop-in's fast paths the draws went through (printed by PetscFinalize)
        L.PetscFinalize.argtypes = []
        L.PetscFinalize()


def _five_point(n, row_coef):
    """dense n^2 x n^2 five-point operator in lexicographic numbering, row_coef(i) = {(i-1), W, C, E, (i+1)} of grid row i; neighbours
    outside the grid are absent (src/solver.c:239-251)"""
    M = np.zeros((n * n, n * n))
    for i in range(n):
        c = row_coef(i)
        for j in range(n):
            r = i * n + j
            if i > 0:
                M[r, r - n] = c[0]
            if j > 0:
                M[r, r - 1] = c[1]
            M[r, r] = c[2]
            if j < n - 1:
                M[r, r + 1] = c[3]
            if i < n - 1:
                M[r, r + n] = c[4]
    return M


def _transfer_pair(nf):
    """dense full weighting ([1 2 1; 2 4 2; 1 2 1] / 16) and bilinear prolongation between nf^2 and ((nf - 1) / 2)^2 unknowns"""
    nc = (nf - 1) // 2
    r1 = np.zeros((nc, nf))
    for i in range(nc):
        r1[i, 2 * i:2 * i + 3] = (0.25, 0.5, 0.25)
    return np.kron(r1, r1), np.kron(2.0 * r1.T, 2.0 * r1.T)


def _device_operator(L, m):
    """what MatView prints for the matrix: the line that names the device operator the drop-in chose"""
    import os
    import sys
    import tempfile
    L.MatView.argtypes = [C.c_void_p, C.c_void_p]
    sys.stdout.flush()
    with tempfile.TemporaryFile() as t:
        saved = os.dup(1)
        os.dup2(t.fileno(), 1)
        try:
            L.MatView(m, None)
        finally:
            os.dup2(saved, 1)
            os.close(saved)
        t.seek(0)
        return t.read().decode()


def nonsymmetric_operators_keep_petsc_semantics(L, orc):
    """Operators the Poisson problem never assembles: a constant five-point matrix with five DISTINCT values and a row-dependent one with
    W != E (tests/coef_cases.py), through MatSetValue.  recognise_stencil / recognise_stencil_rowvar take them (MatView names the device
    operator: no AIJ kernel) and hand the five values to the fused kernels; with the Poisson operators' equal off-diagonals a transposed
    pair on that way would not show.  MatMult, MatResidual / KSPBuildResidual + VecNorm, KSPSolve (Richardson + Jacobi, max_it 1 .. 4 --
    3 takes the three-sweep passes --, zero and nonzero guess), the norm pass followed by an adopting solve, and a two-level step in the
    reference's order (src/solver.c:1531-1546) with a distinct-coefficient coarse operator, against dense numpy.  Tolerance: 1e-11 of the
    vector's magnitude, as random_programs_keep_petsc_semantics; a swapped coefficient moves the result by O(1).
    Sizes: 17^2 and 65^2 unknowns (coarse grids 8^2 / 32^2: even, so the coarse operator and the transfers to it run on the AIJ kernel), and
    15^2 / 63^2 (coarse 7^2 / 31^2: all four recognised, so the fused residual + restriction starts the coarse level with ITS constants and
    the prolongation is fused into the post-smoothing pass)."""
    from coef_cases import distinct_coef, distinct_row_tables
    L.PetscInitialize(None, None, None, None)
    L.PetscOptionsSetValue(None, b"-pc_type", b"jacobi")
    rng = np.random.default_rng(29)
    STENCIL, ROWVAR, AIJ = "matrix-free 5-point stencil\n", "matrix-free 5-point stencil with row-dependent coefficients\n", "assembled AIJ"

    def operator(n, form):
        if form == "constant":
            c = distinct_coef(rng, 2)
            return _five_point(n, lambda i: c)
        ct, _ = distinct_row_tables(rng, n)
        return _five_point(n, lambda i: ct[i])

    def close(got, want, what):
        err = float(np.max(np.abs(got - want)))
        assert err <= 1e-11 * max(1.0, float(np.abs(want).max())), (what, err)

    def norm_close(val, want, what):
        assert abs(val - np.linalg.norm(want)) <= 1e-11 * np.sqrt(want.size) * max(1.0, float(np.abs(want).max())), (what, val, np.linalg.norm(want))

    for n in (17, 65, 15, 63):
        nc = (n - 1) // 2
        Rm, Pm = _transfer_pair(n)
        mR, mP = _assemble(L, Rm), _assemble(L, Pm)
        if nc % 2:
            assert "full weighting" in _device_operator(L, mR) and "bilinear prolongation" in _device_operator(L, mP)
        else:               # (no padded layout for an even grid: the transfers to it are AIJ matrices as well)
            assert AIJ in _device_operator(L, mR) and AIJ in _device_operator(L, mP)
        for form in ("constant", "rowvar"):
            tag = f"n={n} {form}"
            A, Ac = operator(n, form), operator(nc, form)
            assert not np.allclose(A, A.T)
            mA, mAc = _assemble(L, A), _assemble(L, Ac)
            kind = _device_operator(L, mA)
            assert kind.endswith(STENCIL if form == "constant" else ROWVAR) and AIJ not in kind, (tag, kind)
            kind_c = _device_operator(L, mAc)
            if nc % 2:
                assert kind_c.endswith(STENCIL if form == "constant" else ROWVAR) and AIJ not in kind_c, (tag, kind_c)
            else:
                assert AIJ in kind_c, (tag, kind_c)
            nf, ncc = n * n, nc * nc
            d, dc = 1.0 / np.diag(A), 1.0 / np.diag(Ac)
            xv, bv, uv = rng.uniform(-1, 1, nf), rng.uniform(-1, 1, nf), rng.uniform(-1, 1, nf)
            x, b, u, r, rv, y = (C.c_void_p() for _ in range(6))
            uc, bc = C.c_void_p(), C.c_void_p()
            L.MatCreateVecs(mA, C.byref(x), C.byref(b))
            for v in (u, r, rv, y):
                L.VecDuplicate(x, C.byref(v))
            L.MatCreateVecs(mAc, C.byref(uc), C.byref(bc))
            val, V = C.c_double(), C.c_void_p()

            def sweeps(M, dinv, x0, rhs, m, s):
                for _ in range(m):
                    x0 = x0 + s * (dinv * (rhs - M @ x0))
                return x0

            def solver(mat, maxit, scale, guess):
                k = C.c_void_p()
                L.KSPCreate(1, C.byref(k))
                L.KSPSetType(k, b"richardson"); L.KSPSetOperators(k, mat, mat); L.KSPSetNormType(k, 0)
                L.KSPSetTolerances(k, 1e-7, -2.0, -2.0, maxit)
                L.KSPSetFromOptions(k)
                L.KSPRichardsonSetScale(k, scale)
                L.KSPSetInitialGuessNonzero(k, guess)
                return k

            # MatMult, MatResidual + VecNorm
            _set(L, x, xv); _set(L, b, bv)
            L.MatMult(mA, x, y)
            close(_get(L, y, nf), A @ xv, f"{tag}: MatMult")
            L.MatResidual(mA, b, x, r)
            L.VecNorm(r, NORM_2, C.byref(val))
            norm_close(val.value, bv - A @ xv, f"{tag}: MatResidual + VecNorm")
            close(_get(L, r, nf), bv - A @ xv, f"{tag}: MatResidual")
            # KSPSolve: sweeps from the zero guess and from a nonzero one; KSPBuildResidual + VecNorm; the norm pass and the adopting solve
            for maxit in (1, 2, 3, 4):
                for guess in (0, 1):
                    for scale in (0.8, 6.0 / 7.0):
                        t = f"{tag}: max_it={maxit} guess={guess} scale={scale}"
                        k = solver(mA, maxit, scale, guess)
                        _set(L, u, uv); _set(L, b, bv)
                        L.KSPSolve(k, b, u)
                        m1 = sweeps(A, d, uv if guess else np.zeros(nf), bv, maxit, scale)
                        close(_get(L, u, nf), m1, f"{t}: KSPSolve")
                        L.KSPBuildResidual(k, None, r, C.byref(V))
                        L.VecNorm(V, NORM_2, C.byref(val))
                        norm_close(val.value, bv - A @ m1, f"{t}: KSPBuildResidual + VecNorm")
                        L.KSPSolve(k, b, u)                  # with a nonzero guess this adopts the sweeps the norm pass made
                        m2 = sweeps(A, d, m1 if guess else np.zeros(nf), bv, maxit, scale)
                        close(_get(L, u, nf), m2, f"{t}: the solve after the norm pass")
                        close(_get(L, r, nf), bv - A @ m1, f"{t}: r of the norm pass")
                        L.KSPDestroy(C.byref(k))
            # a two-level step in the reference's order, v = (3, 3) and (2, 1)
            for v0, v1, scale in ((3, 3, 0.8), (2, 1, 6.0 / 7.0)):
                t = f"{tag}: two-level step v=({v0},{v1})"
                k0, k1 = solver(mA, v0, scale, 1), solver(mAc, v1, scale, 0)
                _set(L, u, uv); _set(L, b, bv)
                L.KSPSolve(k0, b, u)
                mu = sweeps(A, d, uv, bv, v0, scale)
                L.KSPBuildResidual(k0, None, r, C.byref(V))
                L.MatMult(mR, r, bc)
                mbc = Rm @ (bv - A @ mu)
                L.KSPSolve(k1, bc, uc)
                muc = sweeps(Ac, dc, np.zeros(ncc), mbc, v1, scale)
                L.MatMult(mP, uc, rv)
                L.VecAXPY(u, 1.0, rv)
                L.KSPSolve(k0, b, u)
                mu = sweeps(A, d, mu + Pm @ muc, bv, v0, scale)
                L.KSPBuildResidual(k0, None, r, C.byref(V))
                L.VecNorm(V, NORM_2, C.byref(val))
                norm_close(val.value, bv - A @ mu, f"{t}: norm")
                close(_get(L, u, nf), mu, f"{t}: u")
                close(_get(L, bc, ncc), mbc, f"{t}: coarse right-hand side")
                close(_get(L, uc, ncc), muc, f"{t}: coarse solution")
                close(_get(L, rv, nf), Pm @ muc, f"{t}: prolonged correction")
                L.KSPDestroy(C.byref(k0)); L.KSPDestroy(C.byref(k1))
            for v in (x, b, u, r, rv, y, uc, bc):
                L.VecDestroy(C.byref(v))
            L.MatDestroy(C.byref(mA)); L.MatDestroy(C.byref(mAc))
        L.MatDestroy(C.byref(mR)); L.MatDestroy(C.byref(mP))


def reference_streams(L, fixtures):
    """The drop-in fed with the reference's OWN call stream (tests/golden/ref_assembly.npz through ref_fixtures.load_assembly): every recorded
    MatSetValue / VecSetValue replayed into MatCreateAIJ / MatSetValue / MatAssemblyBegin/End and VecSetValue in the recorded order -- R and P
    and the levels of several grids do not come with ascending columns, as _assemble's matrices do.
    One grid per level (-grids == -levels): MatView must name a recognised device operator for A (5-point stencil; with row-dependent
    coefficients on -mesh 1/2), R (full weighting) and P (bilinear prolongation), and MatMult on a uniform(-1, 1) vector must equal the
    canonical product (oracle/mgo.h: columns ascending, separate multiply and add, the sum starts at 0.0) BIT FOR BIT.
    Levels of several grids (-grids > -levels): 1e-11 * max(1, max|want|), this file's tolerance for operators run as several kernels
    (nonsymmetric_operators_keep_petsc_semantics).  b[0]: VecGetArray returns the recorded values exactly, at npts 65 / 129 too.
    Returns the number of comparisons made."""
    import ref_fixtures as RF
    L.PetscInitialize(None, None, None, None)
    L.VecCreateSeq.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    rng = np.random.default_rng(41)
    names = {RF.KIND_A: {0: "matrix-free 5-point stencil\n", 1: "matrix-free 5-point stencil with row-dependent coefficients\n",
                         2: "matrix-free 5-point stencil with row-dependent coefficients\n"},
             RF.KIND_R: dict.fromkeys((0, 1, 2), "matrix-free full weighting\n"), RF.KIND_P: dict.fromkeys((0, 1, 2), "matrix-free bilinear prolongation\n")}
    done = 0
    for case, c in fixtures.items():
        mesh, npts, grids, levels, _, full = case
        want_b = RF.stream_vector(c)
        n0 = want_b.size
        b = C.c_void_p()
        L.VecCreateSeq(1, n0, C.byref(b))
        row, _, val, _ = RF.stream_select(c, RF.KIND_B, 0)
        for r, v in zip(row.tolist(), val.tolist()):
            L.VecSetValue(b, r, v, INSERT)
        L.VecAssemblyBegin(b); L.VecAssemblyEnd(b)
        assert RF.same_bits(_get(L, b, n0), want_b), (case, "b[0] through VecSetValue / VecGetArray")
        done += 1
        L.VecDestroy(C.byref(b))
        if not full:
            continue
        totals = [int(c["row"][c["obj"] == 32 * RF.KIND_A + l].max()) + 1 for l in range(levels)]
        objs = [int(o) for o in dict.fromkeys(c["obj"].tolist()) if o // 32 != RF.KIND_B]
        for o in objs:
            kind, l = o // 32, o % 32
            sel = np.nonzero(c["obj"] == o)[0]
            assert np.array_equal(sel, np.arange(sel[0], sel[0] + sel.size)), (case, o, "the calls of one matrix are contiguous")
            nr, nc = RF.stream_shape(c, kind, l, totals)
            m = C.c_void_p()
            L.MatCreateAIJ(1, nr, nc, -1, -1, 30, None, 0, None, C.byref(m))
            for r, cc, v, md in zip(c["row"][sel].tolist(), c["col"][sel].tolist(), c["val"][sel].tolist(), c["mode"][sel].tolist()):
                L.MatSetValue(m, r, cc, v, md)
            L.MatAssemblyBegin(m, FINAL); L.MatAssemblyEnd(m, FINAL)
            x, y = C.c_void_p(), C.c_void_p()
            L.MatCreateVecs(m, C.byref(x), C.byref(y))
            xv = rng.uniform(-1, 1, nc)
            _set(L, x, xv)
            L.MatMult(m, x, y)
            got = _get(L, y, nr)
            want = RF.csr_mult_canonical(*RF.stream_csr(c, kind, l, nr), xv)
            tag = (case, "A res pro".split()[kind], l)
            if grids == levels:
                view = _device_operator(L, m)
                assert view.endswith(names[kind][mesh]) and "assembled AIJ" not in view, (tag, view)
                if not RF.same_bits(got, want):
                    q = int(np.nonzero(got != want)[0][0])
                    raise AssertionError((tag, "MatMult differs from the canonical product: first at row", q, float(got[q]).hex(), float(want[q]).hex()))
                done += 2
            else:
                err = float(np.max(np.abs(got - want)))
                assert err <= 1e-11 * max(1.0, float(np.abs(want).max())), (tag, err)
                done += 1
            L.VecDestroy(C.byref(x)); L.VecDestroy(C.byref(y))
            L.MatDestroy(C.byref(m))
    return done


if __name__ == "__main__":      # python tests/shim_semantics.py <shared library> <function name>: one check in a process of its own
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from oracle import Oracle
    lib = type_shim(C.CDLL(sys.argv[1], mode=os.RTLD_LOCAL))
    {"lazy": lazy_temporaries_keep_petsc_semantics, "spec": speculative_sweep_is_adopted_only_when_nothing_changed,
     "keepr": residual_left_deferred_by_the_norm_pass, "tailrec": recorded_coarse_subcycle_keeps_petsc_semantics, "recorder": deferred_values_around_the_recorder, "pcmgtail": pcmg_level_vectors_after_the_tail_launch, "lu": richardson_with_lu_is_damped_not_exact,
     "nonsym": nonsymmetric_operators_keep_petsc_semantics,
     "refstreams": lambda L_, o_: print("reference_streams:", reference_streams(L_, __import__("ref_fixtures").load_assembly()), "comparisons"),
     "random": lambda L_, o_: random_programs_keep_petsc_semantics(L_, o_, seed=int(sys.argv[3]) if len(sys.argv) > 3 else 1,
                                                                   nprog=int(sys.argv[4]) if len(sys.argv) > 4 else 40,
                                                                   extended=len(sys.argv) > 5 and sys.argv[5] == "ext")}[sys.argv[2]](lib, Oracle())
    print("SEMANTICS_OK", sys.argv[2])
