"""ctypes binding of include/mgsolve.h -- the host-side V-cycle driver (C99) over the HIP kernels.

Names follow the reference driver (src/poisson.c:27-138): SetUp -> Assemble (set_rhs_problem) ->
Solve -> Postprocessing (error_norms, solution).  Plumbing only; all work happens in the C library.
"""
import ctypes as C
import enum

import numpy as np

from ._lib import load_mgpetsc


class MgConfig(C.Structure):
    _fields_ = [("dim", C.c_int), ("npts", C.c_int), ("levels", C.c_int), ("v", C.c_int * 2),
                ("maxiter", C.c_int), ("ksp_type", C.c_int), ("scale", C.c_double),
                ("emin", C.c_double), ("emax", C.c_double), ("rtol", C.c_double),
                ("device", C.c_int), ("precision", C.c_int), ("rank", C.c_int), ("nranks", C.c_int),
                ("dist_min_n", C.c_int), ("fuse", C.c_int), ("overlap", C.c_int), ("graph", C.c_int),
                ("pair_min_n", C.c_int), ("slab_chunk", C.c_int), ("mesh", C.c_int), ("pc_type", C.c_int),
                ("line_tail", C.c_int), ("xline_chunk", C.c_int), ("line_chunk", C.c_int)]


class MgError(RuntimeError):
    pass


class Fuse(enum.IntFlag):
    """The bits of Solver(fuse=...), mg_config.fuse: mg_fuse_bits of include/mgsolve.h, which says what each pass is.  The values are ABI
    (plain ints are taken everywhere); value 64 is unassigned, accepted and ignored.  fuse=-1 selects FUSE_AUTO (below): DEFAULT and bit 16 -- and bit 17
    with them in 3-D at npts = 1025."""
    RESNORM = 1
    PROLONG_SWEEP = 2
    RES_RESTRICT = 4
    NORM_SWEEP = 8
    MIXED_CORRECT = 16
    PAIRS = 32
    RES_RESTRICT_SMALL = 128
    COARSE_ZERO_SWEEP = 256
    LDS_TAIL = 512
    SWEEP_RESTRICT = 1024
    ZERO_TRIPLE = 2048
    PROLONG_PAIR = 4096
    TRIPLE_2D = 8192
    PROLONG_PAIR_SLAB = 16384
    CHEBY = 32768
    DEFAULT = (RESNORM | PROLONG_SWEEP | RES_RESTRICT | NORM_SWEEP | MIXED_CORRECT | PAIRS | COARSE_ZERO_SWEEP | LDS_TAIL | SWEEP_RESTRICT |
               ZERO_TRIPLE | PROLONG_PAIR | TRIPLE_2D | PROLONG_PAIR_SLAB | CHEBY)


# MG_FUSE_TRIPLE_MID / MG_FUSE_AUTO of include/mgsolve.h: bit 16 stands beside the enum there and here (the enumerators mirror the C enum one to one)
FUSE_TRIPLE_MID = 65536
FUSE_AUTO = int(Fuse.DEFAULT) | FUSE_TRIPLE_MID
# MG_FUSE_TRIPLE_NORM: bit 17, not part of FUSE_AUTO (fuse=-1 adds it in 3-D at npts = 1025, elsewhere it is opt-in): the 66-byte 3-D fine level,
# post- and pre-smoothing of level 0 as two stacked passes
FUSE_TRIPLE_NORM = 131072


_KSP = {"richardson": 0, "chebyshev": 1}
_PC = {"jacobi": 0, "yline": 1, "xline": 2, "altline": 3}       # the Jacobi-type smoothers (point and line)
_PC_GS = {"rbgs": 4}                                             # the Gauss-Seidel-type smoothers: red-black (mg_pc_type MG_PC_RBGS)


def _lib():
    L = load_mgpetsc()
    if getattr(L, "_mg_sigs", False):
        return L
    vp, i, d = C.c_void_p, C.c_int, C.c_double
    L.mg_config_default.argtypes = [C.POINTER(MgConfig)]
    L.mg_solver_create.restype = i
    L.mg_solver_create.argtypes = [C.POINTER(vp), C.POINTER(MgConfig), vp]
    L.mg_solver_destroy.argtypes = [vp]
    L.mg_last_error.restype = C.c_char_p
    for f in ("mg_solver_set_rhs_problem", "mg_solver_reset", "mg_solver_solve", "mg_solver_sync"):
        getattr(L, f).restype = i
        getattr(L, f).argtypes = [vp]
    L.mg_solver_set_rhs_host.restype = i
    L.mg_solver_set_rhs_host.argtypes = [vp, vp]
    L.mg_solver_cycles.restype = i
    L.mg_solver_cycles.argtypes = [vp, i]
    L.mg_solver_iterations.restype = i
    L.mg_solver_iterations.argtypes = [vp]
    L.mg_solver_bnorm.restype = d
    L.mg_solver_bnorm.argtypes = [vp]
    L.mg_solver_rnorm.restype = C.POINTER(d)
    L.mg_solver_rnorm.argtypes = [vp]
    L.mg_solver_solve_seconds.restype = d
    L.mg_solver_solve_seconds.argtypes = [vp]
    L.mg_solver_num_levels.restype = i
    L.mg_solver_num_levels.argtypes = [vp]
    L.mg_solver_debug_kernel_ctx.restype = vp
    L.mg_solver_debug_kernel_ctx.argtypes = [vp]
    L.mg_solver_tail_level.restype = i
    L.mg_solver_tail_level.argtypes = [vp]
    L.mg_solver_prolong_triple_launches.restype = i
    L.mg_solver_prolong_triple_launches.argtypes = [vp, i]
    L.mg_solver_triple_norm_launches.restype = i
    L.mg_solver_triple_norm_launches.argtypes = [vp]
    L.mg_solver_graph_rerecorded.restype = i
    L.mg_solver_graph_rerecorded.argtypes = [vp]
    L.mg_solver_level_n.restype = i
    L.mg_solver_level_n.argtypes = [vp, i]
    L.mg_solver_level_local_planes.restype = i
    L.mg_solver_level_local_planes.argtypes = [vp, i, C.POINTER(i)]
    L.mg_solver_local_unknowns.restype = C.c_long
    L.mg_solver_local_unknowns.argtypes = [vp]
    L.mg_solver_dof_updates_per_cycle.restype = d
    L.mg_solver_dof_updates_per_cycle.argtypes = [vp]
    L.mg_solver_get_solution.restype = i
    L.mg_solver_get_solution.argtypes = [vp, vp]
    L.mg_solver_error_norms.restype = i
    L.mg_solver_error_norms.argtypes = [vp, C.POINTER(d)]
    L.mg_solver_profile.restype = i
    L.mg_solver_profile.argtypes = [vp, i]
    L.mg_solver_profile_read.restype = i
    L.mg_solver_profile_read.argtypes = [vp, C.POINTER(d), C.POINTER(i)]
    L.mg_solver_profile_read_kind.restype = i
    L.mg_solver_profile_read_kind.argtypes = [vp, i, C.POINTER(d), C.POINTER(i)]
    L.mg_get_ranges.argtypes = [i, i, vp]
    L.mg_grid_n.restype = i
    L.mg_grid_n.argtypes = [i, i]
    L.mg_grid_to_global.restype = C.c_long
    L.mg_grid_to_global.argtypes = [i, i, i, i, i]
    L.mg_global_to_grid.argtypes = [i, i, C.c_long, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.mg_slab_range.restype = i
    L.mg_slab_range.argtypes = [i, i, i, i, i, C.POINTER(i), C.POINTER(i)]
    L._mg_sigs = True
    return L


def _fmg_lib(L):
    """the full-multigrid entry points, bound on first use (a library built without them still serves everything else)"""
    if not getattr(L, "_mg_fmg_sigs", False):
        for f in ("mg_solver_fmg", "mg_solver_solve_fmg"):
            getattr(L, f).restype = C.c_int
            getattr(L, f).argtypes = [C.c_void_p, C.c_int]
        L._mg_fmg_sigs = True
    return L


def _gmres_lib(L):
    """the GMRES entry point, bound on first use like the full-multigrid ones"""
    if not getattr(L, "_mg_gmres_sigs", False):
        L.mg_solver_solve_gmres.restype = C.c_int
        L.mg_solver_solve_gmres.argtypes = [C.c_void_p, C.c_int]
        L._mg_gmres_sigs = True
    return L


def _cg_lib(L):
    """the CG entry points, bound on first use like the GMRES one"""
    if not getattr(L, "_mg_cg_sigs", False):
        L.mg_solver_solve_cg.restype = C.c_int
        L.mg_solver_solve_cg.argtypes = [C.c_void_p]
        L.mg_solver_cg_breakdown.restype = C.c_int
        L.mg_solver_cg_breakdown.argtypes = [C.c_void_p]
        L._mg_cg_sigs = True
    return L


def _cg_mixed_lib(L):
    """the entry point of CG over the fp32 cycle, bound on first use (a library built without mg_cg_mixed.c need not have it)"""
    if not getattr(L, "_mg_cg_mixed_sigs", False):
        L.mg_solver_solve_cg_mixed.restype = C.c_int
        L.mg_solver_solve_cg_mixed.argtypes = [C.c_void_p]
        L._mg_cg_mixed_sigs = True
    return L


def get_ranges(totaln, procs):
    r = np.zeros(procs + 1, dtype=np.int32)
    _lib().mg_get_ranges(totaln, procs, r.ctypes.data_as(C.c_void_p))
    return r


def slab_range(npts, levels_dist, level, rank, nranks):
    a, b = C.c_int(), C.c_int()
    rc = _lib().mg_slab_range(npts, levels_dist, level, rank, nranks, C.byref(a), C.byref(b))
    if rc:
        raise MgError(f"mg_slab_range rc={rc}")
    return a.value, b.value


class Solver:
    """One rank's multigrid solver (whole grid when nranks == 1)."""

    def __init__(self, dim, npts, levels, v=(3, 3), maxiter=100000, ksp_type="richardson", scale=1.0,
                 eigenvalues=(0.0, 0.0), rtol=1.0e-7, device=0, rank=0, nranks=1, comm=None,
                 dist_min_n=0, fuse=-1, overlap=-1, precision="fp64", graph=-1, pair_min_n=0, mesh=0, slab_chunk=-1, pc_type="jacobi",
                 line_chunk=0, xline_chunk=0, line_tail=0):
        self.L = _lib()
        cfg = MgConfig()
        self.L.mg_config_default(C.byref(cfg))
        cfg.dim, cfg.npts, cfg.levels = dim, npts, levels
        cfg.v[0], cfg.v[1] = v
        cfg.maxiter = maxiter
        cfg.ksp_type = _KSP[ksp_type]
        cfg.scale = scale
        cfg.emin, cfg.emax = eigenvalues
        cfg.rtol = rtol
        cfg.device, cfg.rank, cfg.nranks = device, rank, nranks
        cfg.precision = {"fp64": 0, "mixed": 1}[precision]
        cfg.dist_min_n, cfg.fuse, cfg.overlap, cfg.graph = dist_min_n, fuse, overlap, graph
        cfg.pair_min_n = pair_min_n
        cfg.slab_chunk = slab_chunk
        cfg.mesh = mesh
        cfg.pc_type = _PC_GS[pc_type] if pc_type in _PC_GS else _PC[pc_type]      # "yline" / "xline": y- / x-line Jacobi, "altline": y and x sweeps in turn, "rbgs": red-black Gauss-Seidel (2-D, fp64, one rank, Richardson; include/mgsolve.h)
        cfg.xline_chunk = xline_chunk     # c > 0, a multiple of 16: the x-line sweeps in chunks of c columns (four passes per sweep); 0: whole
        cfg.line_chunk = line_chunk       # c >= 2: the y-line sweeps in chunks of c rows (four passes per sweep); 0: whole
        cfg.line_tail = line_tail         # 1: the LDS-resident coarse levels of a line cycle in one launch; 0: by launch
        self.cfg = cfg
        self.h = C.c_void_p()
        self._chk(self.L.mg_solver_create(C.byref(self.h), C.byref(cfg), comm))

    def _chk(self, rc):
        if rc:
            raise MgError(f"rc={rc}: {self.L.mg_last_error().decode()}")

    def close(self):
        if self.h:
            self.L.mg_solver_destroy(self.h)
            self.h = C.c_void_p()

    def set_rhs_problem(self):
        self._chk(self.L.mg_solver_set_rhs_problem(self.h))

    def set_rhs(self, b):
        b = np.ascontiguousarray(b, dtype=np.float64)
        assert b.size == self.local_unknowns
        self._chk(self.L.mg_solver_set_rhs_host(self.h, b.ctypes.data_as(C.c_void_p)))

    def reset(self):
        self._chk(self.L.mg_solver_reset(self.h))

    def solve(self):
        self._chk(self.L.mg_solver_solve(self.h))
        return self.iterations

    def cycles(self, n):
        self._chk(self.L.mg_solver_cycles(self.h, n))

    def fmg(self, nu=1):
        """full multigrid FMG(nu) on the current right-hand side; counts as iteration 1, cycles() continues from its result"""
        self._chk(_fmg_lib(self.L).mg_solver_fmg(self.h, nu))
        return self.iterations

    def solve_fmg(self, nu=1):
        """FMG(nu), then V-cycles under solve()'s stop rule; returns the iteration count (FMG included)"""
        self._chk(_fmg_lib(self.L).mg_solver_solve_fmg(self.h, nu))
        return self.iterations

    def solve_gmres(self, restart=30):
        """restarted GMRES(restart) with the V-cycle as right preconditioner (PETSc's -ksp_type gmres -pc_type mg); returns the number of
        Arnoldi steps; rnorm[k] is the residual estimate after step k"""
        self._chk(_gmres_lib(self.L).mg_solver_solve_gmres(self.h, restart))
        return self.iterations

    def solve_cg(self):
        """conjugate gradients with the V-cycle as preconditioner (PETSc's -ksp_type cg -pc_type mg; uniform mesh, point Jacobi); returns
        the number of CG steps; rnorm[k] is the norm of the recurrence residual after step k.  A breakdown ends the iteration like a stop:
        see cg_breakdown"""
        self._chk(_cg_lib(self.L).mg_solver_solve_cg(self.h))
        return self.iterations

    def solve_cg_mixed(self):
        """solve_cg on a solver created with precision="mixed" (3-D): the fp64 recurrence preconditioned by the fp32 V-cycle,
        M r = (double) Vcycle32((float) r); returns the number of CG steps; rnorm, cg_breakdown and the solution as after solve_cg"""
        self._chk(_cg_mixed_lib(self.L).mg_solver_solve_cg_mixed(self.h))
        return self.iterations

    @property
    def cg_breakdown(self):
        """the step (1-based) in which the last solve_cg or solve_cg_mixed broke down (alpha not finite or <= 0, beta not finite or < 0); 0: it did not"""
        return _cg_lib(self.L).mg_solver_cg_breakdown(self.h)

    def sync(self):
        self._chk(self.L.mg_solver_sync(self.h))

    @property
    def iterations(self):
        return self.L.mg_solver_iterations(self.h)

    @property
    def bnorm(self):
        return self.L.mg_solver_bnorm(self.h)

    @property
    def rnorm(self):
        """absolute residual norms rnorm[0..iterations]"""
        p = self.L.mg_solver_rnorm(self.h)
        return np.array([p[q] for q in range(self.iterations + 1)])

    @property
    def solve_seconds(self):
        return self.L.mg_solver_solve_seconds(self.h)

    @property
    def local_unknowns(self):
        return self.L.mg_solver_local_unknowns(self.h)

    @property
    def dof_updates_per_cycle(self):
        return self.L.mg_solver_dof_updates_per_cycle(self.h)

    @property
    def tail_level(self):
        """the first level that runs inside a tail kernel (fuse bit 9; line_tail for the line smoothers); 0: none"""
        return self.L.mg_solver_tail_level(self.h)

    @property
    def kernel_ctx(self):
        """the kernel context (mgk_ctx *) the solver launches on, as a c_void_p: a test aid (mgk_debug_partials)"""
        return C.c_void_p(self.L.mg_solver_debug_kernel_ctx(self.h))

    def prolong_triple_launches(self, l):
        """launches of the prolongation + three-sweep pass (fuse bit 16, mgk_prolong_jacobi3_f64) on level l since the solver was created"""
        return self.L.mg_solver_prolong_triple_launches(self.h, l)

    @property
    def triple_norm_launches(self):
        """launches of the norm + three-sweep pass of level 0 (fuse bit 17, mgk_jacobi3_sumsq_f64) since the solver was created"""
        return self.L.mg_solver_triple_norm_launches(self.h)

    @property
    def graph_rerecorded(self):
        """recordings of the coarse-level graph thrown away because the pointers of the level that feeds it had changed (0 in every default configuration)"""
        return self.L.mg_solver_graph_rerecorded(self.h)

    def level_n(self, l):
        return self.L.mg_solver_level_n(self.h, l)

    def level_planes(self, l):
        z0 = C.c_int()
        nz = self.L.mg_solver_level_local_planes(self.h, l, C.byref(z0))
        return z0.value, nz

    def solution(self):
        u = np.empty(self.local_unknowns)
        self._chk(self.L.mg_solver_get_solution(self.h, u.ctypes.data_as(C.c_void_p)))
        return u

    def error_norms(self):
        e = (C.c_double * 3)()
        self._chk(self.L.mg_solver_error_norms(self.h, e))
        return np.array(list(e))

    def profile(self, on=True):
        self._chk(self.L.mg_solver_profile(self.h, int(on)))

    def profile_read(self, kind=0):
        """(total ms, launches) of the fine-level launches timed since profile(True): kind 0 plain sweeps,
        kind 1 two-sweeps-in-one-pass launches, kind 2 the three-sweep pass of fuse bit 16 and the norm + three-sweep pass of bit 17"""
        ms, n = C.c_double(), C.c_int()
        self._chk(self.L.mg_solver_profile_read_kind(self.h, kind, C.byref(ms), C.byref(n)))
        return ms.value, n.value
