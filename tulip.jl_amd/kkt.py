"""Host-side mirror of Tulip's KKT interface for the HIP normal-equations backend.

Same names, argument meaning and error behaviour as the reference
(/root/reference/src/KKT/KKT.jl:59-121, src/KKT/Cholmod/spd.jl:5-70); Julia's `update!` /
`solve!` are `update` / `solve` here.  The Julia glue with the same semantics is
tulip.jl_amd/julia/hip.jl.  All numeric work happens in libtlpk.so on the GPU; this module only
validates arguments and maps return codes to exceptions.
"""
import ctypes as C

import numpy as np

from . import _lib

SQRT_EPS = float(np.sqrt(np.finfo(np.float64).eps))


class K1:
    """Normal-equations system, /root/reference/src/KKT/systems.jl:34-54."""


class K2:
    """Augmented system, /root/reference/src/KKT/systems.jl:12-31 -- the reference's default for Float64
    (KKT.jl:134-141, Cholmod/sqd.jl).  On the device: signed Cholesky P K P' = L S L' of the quasi-definite
    matrix [-(Theta^-1 + Rp) A'; A Rd]."""


class DimensionMismatch(ValueError):
    """Julia's DimensionMismatch (spd.jl:26-34)."""


class PosDefException(ArithmeticError):
    """Julia's PosDefException (spd.jl:47); caught by the IPM to bump regularisations
    (/root/reference/src/IPM/HSD/step.jl:39-48)."""

    def __init__(self, info=0):
        super().__init__(f"matrix is not positive definite; Cholesky factorization failed (column {info})")
        self.info = info


class OutOfMemoryError(MemoryError):
    """Julia's OutOfMemoryError -> Trm_MemoryLimit (/root/reference/src/IPM/HSD/HSD.jl:327-329)."""


class _BackendOptions:
    """What the shared code of the solver objects (HIPNormalEquations, HIPDenseNormalEquations) and the test tools read from any
    backend object, with the value that means "not used".  A backend class sets what it offers; a field that one of them grows gets
    its default here, so that the others keep working."""

    device = 0
    profile = False
    mem_budget_bytes = 0
    ordering, relax = _lib.ORDER_AMD, True
    rank, nranks, ngpus, devices = 0, 1, 1, None
    streams, refine = 0, 0
    row_block = user_perm = None
    detect_blocks, max_link_rows = False, 0
    dense_cols, max_dense_cols, dense_col_min = None, 0, 0


class Backend(_BackendOptions):
    """`TlpHIP.Backend`: selects the HIP solver, the analogue of `TlpCholmod.Backend`
    (/root/reference/src/KKT/Cholmod/cholmod.jl:18).

    row_block: optional block-angular structure (length m; block id >= 0 or -1 for a linking
    row) -- Tulip's structured-matrix hook (parameters.jl:11 MatrixFactory -> KKT.setup dispatch) --
    or "auto": the library finds the structure of the matrix it is given (tlpk_detect_blocks).  An explicit
    map indexes the rows of the matrix KKT.setup receives, i.e. it is only meaningful without presolve
    (Tulip's presolve removes and renumbers rows, model.jl:88-131); "auto" works on the presolved matrix.

    dense_cols (K1, one GPU): None = off; "auto" = columns with more than `dense_col_min` entries (0 = 1000) stay out of
    A*D*A' and become augmented nodes of a quasi-definite system of order m + k (at most `max_dense_cols`, 0 = 1024, the
    densest first); a sequence of column indices additionally marks those columns (only meaningful without presolve).
    """

    def __init__(self, device=0, ordering="amd", relax=True, row_block=None, user_perm=None,
                 profile=False, rank=0, nranks=1, mem_budget_bytes=0, streams=0, ngpus=1, devices=None, refine=0,
                 max_link_rows=0, dense_cols=None, max_dense_cols=0, dense_col_min=0):
        self.device = device
        self.ordering = {"amd": _lib.ORDER_AMD, "natural": _lib.ORDER_NATURAL, "user": _lib.ORDER_USER}[ordering]
        self.relax = bool(relax)
        self.detect_blocks = isinstance(row_block, str)
        if self.detect_blocks:
            if row_block != "auto":
                raise ValueError("row_block: a vector of block ids, None, or 'auto'")
            row_block = None
        self.max_link_rows = int(max_link_rows)
        self.row_block = None if row_block is None else np.ascontiguousarray(row_block, dtype=np.int64)
        self.user_perm = None if user_perm is None else np.ascontiguousarray(user_perm, dtype=np.int64)
        self.profile = bool(profile)
        self.rank, self.nranks = int(rank), int(nranks)
        self.mem_budget_bytes = int(mem_budget_bytes)
        self.streams = int(streams)            # 0 = auto (2 concurrent block groups), 1 = single group
        self.refine = int(refine)              # iterative-refinement steps per solve (0 = the reference's behaviour; K1; one rank or ngpus > 1 -- sharded handles: refine_local / refine_finish)
        # single-process multi-GPU (block-angular LPs): one handle shards the diagonal blocks over `ngpus` devices
        self.ngpus = int(ngpus)
        self.devices = None if devices is None else np.ascontiguousarray(devices, dtype=np.int32)
        if isinstance(dense_cols, str) and dense_cols != "auto":
            raise ValueError("dense_cols: None, 'auto', or column indices")
        self.dense_cols = dense_cols if dense_cols is None or isinstance(dense_cols, str) else np.unique(np.asarray(dense_cols, dtype=np.int64))
        self.max_dense_cols = int(max_dense_cols)
        self.dense_col_min = int(dense_col_min)


class DenseBackend(_BackendOptions):
    """`TlpHIP.DenseBackend`: the analogue of `TlpDense.Backend` (/root/reference/src/KKT/Dense/lapack.jl:17) -- `A` is a dense
    matrix, `A*D*A' + Rd` is formed on the fp64 matrix cores into one dense front and factorised by the blocked dense
    Cholesky of the sparse handles.  K1 only, one GPU; no pattern of `A*D*A'` and no assembly lists are built."""

    def __init__(self, device=0, profile=False, mem_budget_bytes=0):
        self.device = int(device)
        self.profile = bool(profile)
        self.mem_budget_bytes = int(mem_budget_bytes)


class KrylovBackend(_BackendOptions):
    """`TlpHIP.KrylovBackend`: the analogue of `TlpKrylov.Backend` with `Krylov.CgSolver` (the reference's src/KKT/Krylov/spd.jl) --
    no analysis and no factor: every solve runs conjugate gradients on `A*D*A' + Rd` on the device, matrix-free.  K1 only, one GPU.
    precond: None (the reference) or "jacobi" (the diagonal of `A*D*A' + Rd`, rebuilt by every update); itmax = 0: 2 m; atol = rtol = 0:
    sqrt(eps).  A solve that stops at `itmax` still returns its last iterate, as the reference does: `stats()["krylov_converged"]` tells.

    method="minres": `Krylov.MinresSolver` (src/KKT/Krylov/sid.jl) -- MINRES on the augmented system `[-E A'; A Rd]`, K2 only
    (`setup(A, K2(), KrylovBackend(method="minres"))`).  precond "jacobi" is then the block diagonal `diag(E_j, sum_j A_ij^2 / E_j + Rd_i)`
    and itmax = 0 means 2 (m + n).

    method="tricg": `Krylov.TricgSolver` (src/KKT/Krylov/sqd.jl) -- TriCG on the symmetric quasi-definite form `[Rd A; A' -E]`, K2 only.
    precond must be None (`E` and `Rd` are the method's inner products); itmax = 0 means 2 (m + n).  An update with an `E_j <= 0` or an
    `Rd_i <= 0` raises PosDefException (`stats()["fail_col"]`: `j`, or `n + i`) and leaves the handle usable.

    What a handle of this backend reports: `stats()` -- `krylov_iters`, `krylov_iters_total`, `krylov_converged`, `krylov_resid0`, `krylov_resid`,
    `launches_solve` of the last solve; `symbolic("krylov_unsolved")` -- solves since create that did not meet the stopping rule.
    `solve2_device` runs its two right-hand sides through ONE sequence of launches, each bit for bit as `solve_device` would solve it alone and each
    stopping on its own; afterwards `stats()` reads as after the two solves one behind the other (the last-solve fields describe the second
    right-hand side, `launches_solve` is that of the pair) and
      `symbolic("krylov_pair")`        -> [paired solves since create, pairs that fell back to two solves since create, iterations of right-hand side 0
                                          and of 1 in the last pair, their outcome codes (1 solved, 2 itmax, 3 breakdown), rounds of launches enqueued]
      `symbolic_f64("krylov_pair_resid")` -> [resid0, resid of right-hand side 0, resid0, resid of 1] of the last pair.
    The vectors of the second right-hand side are allocated by the first pair (`stats()["device_bytes"]` grows then); if they would cross
    `mem_budget_bytes`, or with `TLPK_KRYLOV_PAIR=0` in the environment at setup, a pair is two solves."""

    def __init__(self, device=0, precond=None, itmax=0, atol=0.0, rtol=0.0, profile=False, mem_budget_bytes=0, method="cg"):
        if precond not in (None, "none", "jacobi"):
            raise ValueError("precond: None or 'jacobi'")
        if method not in ("cg", "minres", "tricg"):
            raise ValueError("method: 'cg' (K1), 'minres' or 'tricg' (K2)")
        if method == "tricg" and precond not in (None, "none"):
            raise ValueError("method='tricg' takes no preconditioner: precond must be None")
        self.method = method
        self.device = int(device)
        self.precond = _lib.PRECOND_JACOBI if precond == "jacobi" else _lib.PRECOND_NONE
        self.itmax = int(itmax)
        self.atol, self.rtol = float(atol), float(rtol)
        self.profile = bool(profile)
        self.mem_budget_bytes = int(mem_budget_bytes)


def detect_blocks(A, max_link_rows=0):
    """tlpk_detect_blocks on a scipy sparse matrix: (row_block, n_blocks, n_link); n_blocks == 1: no block structure."""
    import scipy.sparse as sp
    A = sp.csc_matrix(A)
    m, n = A.shape
    colptr = np.ascontiguousarray(A.indptr, dtype=np.int64); rowval = np.ascontiguousarray(A.indices, dtype=np.int64)
    rb = np.zeros(max(m, 1), dtype=np.int64)
    nb, nl = C.c_int64(1), C.c_int64(0)
    rc = _lib.lib().tlpk_detect_blocks(m, n, _lib.as_p64(colptr), _lib.as_p64(rowval), 0, int(max_link_rows), _lib.as_p64(rb),
                                       C.byref(nb), C.byref(nl))
    _raise_for(rc, None, "tlpk_detect_blocks: ")
    return rb[:m], int(nb.value), int(nl.value)


def _raise_for(code, handle=None, what=""):
    if code == _lib.OK:
        return
    msg = _lib.strerror(code)
    # a failed create returns no handle: its diagnostic is tlpk_last_create_error()
    detail = _lib.lib().tlpk_last_error(handle).decode() if handle else (_lib.lib().tlpk_last_create_error().decode() if what.startswith("KKT.setup") else "")
    if detail:
        msg = f"{msg}: {detail}"
    if code == _lib.NOT_POSDEF:
        raise PosDefException(0)
    if code == _lib.BADARG:
        raise DimensionMismatch(f"{what}{msg}")
    if code in (_lib.OOM, _lib.TOO_LARGE):
        raise OutOfMemoryError(msg)
    raise RuntimeError(f"{what}{msg} (code {code})")


class HIPNormalEquations:
    """`HIPNormalEquations <: AbstractKKTSolver{Float64}` -- the counterpart of
    `CholmodSolver{Float64,K1}` (/root/reference/src/KKT/Cholmod/cholmod.jl:46-60)."""

    def __init__(self, A, backend_, system=_lib.SYSTEM_K1):
        import scipy.sparse as sp
        if not sp.issparse(A):
            A = sp.csc_matrix(np.asarray(A, dtype=np.float64))     # cholmod.jl:65 convert(SparseMatrixCSC, A)
        A = A.tocsc()
        A.sort_indices()
        self.m, self.n = A.shape
        self.A = A                                                # stored by reference, never mutated
        L = _lib.lib()
        opt = _lib.Options()
        L.tlpk_default_options(C.byref(opt))
        opt.device = backend_.device
        opt.ordering = backend_.ordering
        opt.relax = int(backend_.relax)
        opt.profile = int(backend_.profile)
        opt.rank, opt.nranks = backend_.rank, backend_.nranks
        opt.mem_budget_bytes = backend_.mem_budget_bytes
        opt.streams = backend_.streams
        opt.refine_steps = backend_.refine
        opt.detect_blocks = int(backend_.detect_blocks)
        opt.max_link_rows = int(backend_.max_link_rows)
        opt.system = system
        self.system = system
        self._keep = []
        if backend_.row_block is not None:
            if backend_.row_block.shape != (self.m,):
                raise DimensionMismatch(f"length(row_block)={backend_.row_block.shape[0]} but A has m={self.m}")
            opt.row_block = _lib.as_p64(backend_.row_block)
            self._keep.append(backend_.row_block)
        if backend_.user_perm is not None:
            nperm = self.m + self.n if system == _lib.SYSTEM_K2 else self.m      # the nodes of the factored system
            if backend_.ordering == _lib.ORDER_USER and backend_.user_perm.shape != (nperm,):
                raise DimensionMismatch(f"length(user_perm)={backend_.user_perm.size} but the system has {nperm} nodes")
            opt.user_perm = _lib.as_p64(backend_.user_perm)
            self._keep.append(backend_.user_perm)
        if isinstance(backend_, KrylovBackend):
            if backend_.method == "cg" and system != _lib.SYSTEM_K1:
                raise TypeError("the Krylov backend solves the normal equations (K1) only (method='minres' and method='tricg' solve K2)")
            if backend_.method != "cg" and system != _lib.SYSTEM_K2:
                raise TypeError(f"KrylovBackend(method='{backend_.method}') solves the augmented system (K2) only")
            opt.krylov = {"cg": _lib.KRYLOV_CG, "minres": _lib.KRYLOV_MINRES, "tricg": _lib.KRYLOV_TRICG}[backend_.method]
            opt.krylov_precond = backend_.precond
            opt.krylov_itmax = backend_.itmax
            opt.krylov_atol, opt.krylov_rtol = backend_.atol, backend_.rtol
        dense = backend_.dense_cols
        if dense is not None:
            opt.dense_cols = 1
            opt.max_dense_cols = backend_.max_dense_cols
            opt.dense_col_min = backend_.dense_col_min
            if not isinstance(dense, str):
                if dense.size and (dense[0] < 0 or dense[-1] >= self.n):
                    raise DimensionMismatch(f"dense_cols: column index out of range for n={self.n}")
                flags = np.zeros(max(self.n, 1), dtype=np.int64)
                flags[dense] = 1
                opt.col_dense = _lib.as_p64(flags)
                self._keep.append(flags)           # read by tlpk_create only; kept alive with the handle all the same
        colptr = np.ascontiguousarray(A.indptr, dtype=np.int64)
        rowval = np.ascontiguousarray(A.indices, dtype=np.int64)
        nzval = np.ascontiguousarray(A.data, dtype=np.float64)
        self._h = C.c_void_p()
        if backend_.ngpus > 1:
            if backend_.devices is not None and backend_.devices.shape != (backend_.ngpus,):
                raise DimensionMismatch("devices must list ngpus ordinals")
            dv = None if backend_.devices is None else backend_.devices.ctypes.data_as(C.POINTER(C.c_int32))
            rc = L.tlpk_create_multi(C.byref(self._h), self.m, self.n, _lib.as_p64(colptr), _lib.as_p64(rowval),
                                     _lib.as_pd(nzval), 0, C.byref(opt), backend_.ngpus, dv)
        else:
            rc = L.tlpk_create(C.byref(self._h), self.m, self.n, _lib.as_p64(colptr), _lib.as_p64(rowval),
                               _lib.as_pd(nzval), 0, C.byref(opt))
        if rc != _lib.OK:
            h = self._h if self._h else None
            try:
                _raise_for(rc, h, "KKT.setup: ")
            finally:
                if self._h:
                    L.tlpk_destroy(self._h)
                    self._h = C.c_void_p()
        self.backend_options = backend_

    # -- introspection --
    def stats(self):
        st = _lib.Stats()
        _lib.lib().tlpk_info(self._h, C.byref(st))
        return st.as_dict()

    def kernel_times(self):
        kt = _lib.KernelTimes()
        _lib.lib().tlpk_kernel_timing(self._h, C.byref(kt))
        return kt.as_dict()

    def set_profile(self, on):
        _lib.lib().tlpk_set_profile(self._h, int(bool(on)))

    # -- split-phase entry points for block-angular sharding (include/tlpk.h) --
    def update_local(self, d_theta, d_regP, d_regD):
        _raise_for(_lib.lib().tlpk_update_local(self._h, d_theta, d_regP, d_regD), self._h)

    def update_finish(self):
        _raise_for(_lib.lib().tlpk_update_finish(self._h), self._h)

    def solve_local(self, d_xip, d_xid):
        _raise_for(_lib.lib().tlpk_solve_local(self._h, d_xip, d_xid), self._h)

    def solve_finish(self, d_dx, d_dy, d_xid):
        _raise_for(_lib.lib().tlpk_solve_finish(self._h, d_dx, d_dy, d_xid), self._h)

    def solve2_local(self, d_xip0, d_xid0, d_xip1, d_xid1):
        """First half of a pair of solves on a sharded handle (then: all-reduce root_rhs() and root_rhs2(), solve2_finish)."""
        _raise_for(_lib.lib().tlpk_solve2_local(self._h, d_xip0, d_xid0, d_xip1, d_xid1), self._h)

    def solve2_finish(self, d_dx0, d_dy0, d_xid0, d_dx1, d_dy1, d_xid1):
        _raise_for(_lib.lib().tlpk_solve2_finish(self._h, d_dx0, d_dy0, d_xid0, d_dx1, d_dy1, d_xid1), self._h)

    def root_rhs2(self):
        """(device address, count) of the root right-hand side of the SECOND system of a pair."""
        p = C.c_void_p(); n = C.c_int64()
        _raise_for(_lib.lib().tlpk_root_rhs2(self._h, C.byref(p), C.byref(n)), self._h)
        return p.value, n.value

    def refine_local(self, d_dx, d_dy, d_xip, d_xid):
        """First half of one iterative-refinement step on a sharded handle (then: all-reduce root_rhs(), refine_finish)."""
        _raise_for(_lib.lib().tlpk_refine_local(self._h, d_dx, d_dy, d_xip, d_xid), self._h)

    def refine_finish(self, d_dx, d_dy):
        _raise_for(_lib.lib().tlpk_refine_finish(self._h, d_dx, d_dy), self._h)

    def root_panel(self):
        """(device address, count) of the root (linking) panel to all-reduce after update_local."""
        p = C.c_void_p(); n = C.c_int64()
        _raise_for(_lib.lib().tlpk_root_panel(self._h, C.byref(p), C.byref(n)), self._h)
        return (p.value or 0), n.value

    def root_copy(self, which, direction, d_buf):
        """which: 'panel' | 'rhs' | 'rhs2' (second system of a pair); direction: 'out' (library -> d_buf) | 'in'; async on the stream."""
        rc = _lib.lib().tlpk_root_copy(self._h, {"panel": 0, "rhs": 1, "rhs2": 2}[which], 0 if direction == "out" else 1, d_buf)
        _raise_for(rc, self._h)

    def root_rhs(self):
        p = C.c_void_p(); n = C.c_int64()
        _raise_for(_lib.lib().tlpk_root_rhs(self._h, C.byref(p), C.byref(n)), self._h)
        return (p.value or 0), n.value

    def perm(self):
        """perm[new] = old.  K1: the m rows of S; K2: the n + m nodes of the augmented matrix (variables 0..n-1,
        constraints n..n+m-1)."""
        p = np.empty(self.m + self.n if self.system == _lib.SYSTEM_K2 else self.m, dtype=np.int64)
        _lib.lib().tlpk_get_perm(self._h, _lib.as_p64(p))
        return p

    def symbolic(self, what):
        return _lib.symbolic_array(self._h, what)

    def symbolic_f64(self, what):
        """tlpk_symbolic_get_f64: "pair_w", "krylov_pair_resid" (KrylovBackend)"""
        return _lib.symbolic_array_f64(self._h, what)

    def factor_panels(self):
        st = self.stats()
        buf = np.empty(max(st["nnzL_stored"], 1))
        _raise_for(_lib.lib().tlpk_get_factor(self._h, _lib.as_pd(buf), buf.size), self._h)
        return buf[:st["nnzL_stored"]]

    # -- device-pointer entry points (arguments: integer device addresses) --
    def update_device(self, d_theta, d_regP, d_regD):
        _raise_for(_lib.lib().tlpk_update_device(self._h, d_theta, d_regP, d_regD), self._h)

    def update_device_async(self, d_theta, d_regP, d_regD):
        """tlpk_update_device_async: no wait; the verdict (PosDefException) comes from the next sync()."""
        _raise_for(_lib.lib().tlpk_update_device_async(self._h, d_theta, d_regP, d_regD), self._h)

    def solve_device(self, d_dx, d_dy, d_xip, d_xid, sync=True):
        _raise_for(_lib.lib().tlpk_solve_device(self._h, d_dx, d_dy, d_xip, d_xid), self._h)
        if sync:
            _raise_for(_lib.lib().tlpk_sync(self._h), self._h)

    def solve2_device(self, d_dx0, d_dy0, d_xip0, d_xid0, d_dx1, d_dy1, d_xip1, d_xid1, sync=True):
        """Two right-hand sides in one pass over the factor (tlpk_solve2_device); bit-identical to two solve_device calls.  A KrylovBackend handle runs
        both iterations through one sequence of launches (see there).  The four outputs are distinct from each other and from every input; the inputs may
        alias each other."""
        _raise_for(_lib.lib().tlpk_solve2_device(self._h, d_dx0, d_dy0, d_xip0, d_xid0, d_dx1, d_dy1, d_xip1, d_xid1), self._h)
        if sync:
            _raise_for(_lib.lib().tlpk_sync(self._h), self._h)

    def polish_device(self, d_dx, d_dy, d_xip, d_xid, steps=1, sync=True):
        """tlpk_polish_device: up to `steps` guarded refinement steps on (dx, dy) in place, K1 or K2; steps=0 measures only (polish_report)."""
        _raise_for(_lib.lib().tlpk_polish_device(self._h, d_dx, d_dy, d_xip, d_xid, int(steps)), self._h, "polish: ")
        if sync:
            _raise_for(_lib.lib().tlpk_sync(self._h), self._h)

    def polish2_device(self, d_dx0, d_dy0, d_xip0, d_xid0, d_dx1, d_dy1, d_xip1, d_xid1, steps=1, sync=True):
        """tlpk_polish2_device: two systems in one pass over A and one paired pass over L per step; each ends bit for bit as polish_device leaves it alone.
        Buffer rules as for solve2_device."""
        _raise_for(_lib.lib().tlpk_polish2_device(self._h, d_dx0, d_dy0, d_xip0, d_xid0, d_dx1, d_dy1, d_xip1, d_xid1, int(steps)), self._h, "polish: ")
        if sync:
            _raise_for(_lib.lib().tlpk_sync(self._h), self._h)

    def polish(self, dx, dy, xi_p, xi_d, steps=1):
        """tlpk_polish on host arrays: dx, dy (the output of `solve`, or any other approximation) are corrected in place; blocks.  Returns polish_report()."""
        if not (isinstance(dx, np.ndarray) and isinstance(dy, np.ndarray) and dx.dtype == np.float64
                and dy.dtype == np.float64 and dx.flags.c_contiguous and dy.flags.c_contiguous):
            raise TypeError("dx, dy must be contiguous float64 numpy vectors (modified in place)")
        if dx.shape != (self.n,):
            raise DimensionMismatch(f"length(dx)={dx.shape[0]} but KKT solver has n={self.n}")
        if dy.shape != (self.m,):
            raise DimensionMismatch(f"length(dy)={dy.shape[0]} but KKT solver has m={self.m}")
        xp = _vec(xi_p, "ξp", ("m", self.m), "")
        xd = _vec(xi_d, "ξd", ("n", self.n), "")
        rc = _lib.lib().tlpk_polish(self._h, _lib.as_pd(dx), _lib.as_pd(dy), _lib.as_pd(xp), _lib.as_pd(xd), int(steps))
        _raise_for(rc, self._h, "polish: ")
        return self.polish_report()

    def polish_report(self):
        """What the last polish call did (after a sync): per system the steps asked / accepted / rejected and |r1|inf, |r2|inf at entry and of what was kept;
        `bytes`: the device memory the first call allocated.  All zero before the first call."""
        cnt = _lib.symbolic_array(self._h, "polish"); res = _lib.symbolic_array_f64(self._h, "polish_resid")
        sides = [{"asked": int(cnt[3 * s]), "accepted": int(cnt[3 * s + 1]), "rejected": int(cnt[3 * s + 2]),
                  "r1_in": float(res[4 * s]), "r2_in": float(res[4 * s + 1]), "r1": float(res[4 * s + 2]), "r2": float(res[4 * s + 3])} for s in range(2)]
        return {"sides": sides, "bytes": int(_lib.symbolic_array(self._h, "polish_bytes")[0])}

    def sync(self):
        _raise_for(_lib.lib().tlpk_sync(self._h), self._h)

    def stream_ptr(self):
        """hipStream_t of the handle (an integer address), e.g. for torch.cuda.ExternalStream."""
        return _lib.lib().tlpk_stream(self._h) or 0

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().tlpk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):                       # the Julia glue does this in a finalizer
        try:
            self.close()
        except Exception:
            pass


class HIPDenseNormalEquations(HIPNormalEquations):
    """`setup(A::Matrix{Float64}, ::K1, ::DenseBackend)`: a handle of `tlpk_create_dense`; everything else is inherited."""

    def __init__(self, A, backend_):
        import scipy.sparse as sp
        if sp.issparse(A):
            raise TypeError("DenseBackend takes a dense 2-D array; a sparse matrix goes to Backend")
        A = np.asarray(A)
        if A.ndim != 2:
            raise TypeError("DenseBackend takes a 2-D array")
        # column-major float64: a Fortran-ordered array (or a view into one with unit row stride) is passed as it is, anything else is copied once
        s0, s1 = A.strides
        if not (A.dtype == np.float64 and A.flags.aligned and A.shape[0] >= 1 and s0 == 8 and (A.shape[1] <= 1 or (s1 % 8 == 0 and s1 >= 8 * A.shape[0]))):
            A = np.asfortranarray(A, dtype=np.float64)
        self.m, self.n = A.shape
        lda = max(self.m, 1) if self.n <= 1 else A.strides[1] // 8
        self.A = A                                                # stored by reference, never mutated
        self.system = _lib.SYSTEM_K1
        self._keep = []
        L = _lib.lib()
        opt = _lib.Options()
        L.tlpk_default_options(C.byref(opt))
        opt.device = backend_.device
        opt.profile = int(backend_.profile)
        opt.mem_budget_bytes = backend_.mem_budget_bytes
        self._h = C.c_void_p()
        rc = L.tlpk_create_dense(C.byref(self._h), self.m, self.n, A.ctypes.data_as(_lib.pd), lda, C.byref(opt))
        if rc != _lib.OK:
            h = self._h if self._h else None
            try:
                _raise_for(rc, h, "KKT.setup: ")
            finally:
                if self._h:
                    L.tlpk_destroy(self._h)
                    self._h = C.c_void_p()
        self.backend_options = backend_


def setup(A, system=None, backend_=None):
    """KKT.setup(A, ::K1, ::TlpHIP.Backend)  (KKT.jl:59, spd.jl:5-20).  Runs the analyse phase on
    the host and uploads the symbolic structures; skips the throw-away numeric factorisation of
    spd.jl:14-17."""
    if isinstance(backend_, DenseBackend):
        if not (system is None or isinstance(system, K1) or system is K1):
            raise TypeError("the dense backend solves the normal equations (K1) only")
        return HIPDenseNormalEquations(A, backend_)
    if system is None or isinstance(system, K1) or system is K1:
        return HIPNormalEquations(A, backend_ or Backend())
    if isinstance(system, K2) or system is K2:
        return HIPNormalEquations(A, backend_ or Backend(), system=_lib.SYSTEM_K2)
    raise TypeError("the HIP backend solves the normal equations (K1) or the augmented system (K2)")


def _vec(x, name, length, what):
    a = np.ascontiguousarray(x, dtype=np.float64)
    if a.ndim != 1 or a.shape[0] != length[1]:
        raise DimensionMismatch(f"length({name})={a.shape[0] if a.ndim == 1 else a.shape} "
                                f"but KKT solver has {length[0]}={length[1]}{what}")
    return a


def update(kkt, theta_inv, regP, regD):
    """KKT.update!(kkt, θinv, regP, regD) -> nothing  (KKT.jl:65-83, spd.jl:22-50).
    Raises DimensionMismatch (spd.jl:26-34) or PosDefException (spd.jl:47)."""
    th = _vec(theta_inv, "θ", ("n", kkt.n), ".")
    rp = _vec(regP, "regP", ("n", kkt.n), "")
    rd = _vec(regD, "regD", ("m", kkt.m), "")
    rc = _lib.lib().tlpk_update(kkt._h, _lib.as_pd(th), _lib.as_pd(rp), _lib.as_pd(rd))
    _raise_for(rc, kkt._h, "KKT.update!: ")
    return None


def solve(dx, dy, kkt, xi_p, xi_d):
    """KKT.solve!(dx, dy, kkt, ξp, ξd) -> nothing  (KKT.jl:85-100, spd.jl:52-70).
    dx, dy are overwritten in place; ξp, ξd are read-only."""
    if not (isinstance(dx, np.ndarray) and isinstance(dy, np.ndarray) and dx.dtype == np.float64
            and dy.dtype == np.float64 and dx.flags.c_contiguous and dy.flags.c_contiguous):
        raise TypeError("dx, dy must be contiguous float64 numpy vectors (modified in place)")
    if dx.shape != (kkt.n,):
        raise DimensionMismatch(f"length(dx)={dx.shape[0]} but KKT solver has n={kkt.n}")
    if dy.shape != (kkt.m,):
        raise DimensionMismatch(f"length(dy)={dy.shape[0]} but KKT solver has m={kkt.m}")
    xp = _vec(xi_p, "ξp", ("m", kkt.m), "")
    xd = _vec(xi_d, "ξd", ("n", kkt.n), "")
    rc = _lib.lib().tlpk_solve(kkt._h, _lib.as_pd(dx), _lib.as_pd(dy), _lib.as_pd(xp), _lib.as_pd(xd))
    _raise_for(rc, kkt._h, "KKT.solve!: ")
    return None


def set_values(kkt, A_or_data):
    """New numerical values on the analysed pattern (tlpk_set_values / tlpk_set_values_dense): the handle keeps its analysis and is
    NOT factored afterwards -- `update` before the next `solve`.  Sparse handles take a scipy matrix whose sorted CSC pattern
    equals the handle's (otherwise DimensionMismatch) or a 1-D array of nnz(A) values in that order; dense-matrix handles a 2-D
    array of the handle's shape.  `kkt.A` is replaced by a matrix with the new values (the caller's old matrix is not modified)."""
    import scipy.sparse as sp
    L = _lib.lib()
    if isinstance(kkt, HIPDenseNormalEquations):
        if sp.issparse(A_or_data):
            raise DimensionMismatch("set_values: a dense-matrix handle takes a 2-D array")
        A = np.asarray(A_or_data)
        if A.ndim != 2 or A.shape != (kkt.m, kkt.n):
            raise DimensionMismatch(f"set_values: array of shape {A.shape} but the handle has a {kkt.m} x {kkt.n} matrix")
        A = np.asfortranarray(A, dtype=np.float64)
        _raise_for(L.tlpk_set_values_dense(kkt._h, A.ctypes.data_as(_lib.pd), max(kkt.m, 1)), kkt._h, "set_values: ")
        kkt.A = A
        return None
    if sp.issparse(A_or_data):
        B = A_or_data.tocsc()
        if B is A_or_data:
            B = B.copy()
        B.sort_indices()
        if B.shape != kkt.A.shape or not np.array_equal(B.indptr, kkt.A.indptr) or not np.array_equal(B.indices, kkt.A.indices):
            raise DimensionMismatch("set_values: the matrix does not have the pattern the handle was analysed on")
        data = np.ascontiguousarray(B.data, dtype=np.float64)
    else:
        data = np.ascontiguousarray(A_or_data, dtype=np.float64)
        if data.ndim != 1:
            raise DimensionMismatch("set_values: a sparse handle takes a scipy matrix or a 1-D array of nnz(A) values")
    _raise_for(L.tlpk_set_values(kkt._h, _lib.as_pd(data), data.shape[0]), kkt._h, "set_values: ")
    kkt.A = sp.csc_matrix((data.copy(), kkt.A.indices, kkt.A.indptr), shape=kkt.A.shape)
    return None


def block_skip(kkt, mask):
    """tlpk_block_skip: leave diagonal blocks out of the following `update` / `solve` calls.  mask: one entry per block of the handle's
    `row_block` (non-zero = skipped), or None = no mask.  The skipped blocks' panels keep every bit, the other blocks' factor and their
    segments of dx / dy are those of an unmasked call bit for bit; the skipped segments of dx / dy are unspecified (finite).  A block
    that is solved must have been factorised by the last update that touched it.  Handles with linking rows, without row_block, with
    refine > 0, batch-loaded, multi-device, sharded, dense, Krylov or dense_cols handles raise (TLPK_BADARG)."""
    L = _lib.lib()
    nb = int(kkt.stats()["n_blocks"])
    if mask is None:
        rc = L.tlpk_block_skip(kkt._h, None, nb)
    else:
        m8 = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m8.ndim != 1:
            raise DimensionMismatch("block_skip: the mask is a vector with one entry per block")
        rc = L.tlpk_block_skip(kkt._h, _lib.as_pu8(m8), m8.shape[0])
    _raise_for(rc, kkt._h, "block_skip: ")
    return None


def set_values_device(kkt, d_nzval, length):
    """tlpk_set_values_device: the values are in device memory (integer address), the refresh is enqueued on the handle's stream.
    `kkt.A` is NOT updated (the values never reach the host)."""
    _raise_for(_lib.lib().tlpk_set_values_device(kkt._h, d_nzval, int(length)), kkt._h, "set_values: ")


def arithmetic(kkt):
    """KKT.arithmetic (KKT.jl:107)."""
    return np.float64


def backend(kkt):
    """KKT.backend (KKT.jl:114) -- printed in the IPM log banner (HSD.jl:227-229)."""
    name = _lib.lib().tlpk_backend_name().decode()
    be = getattr(kkt, "backend_options", None)
    if isinstance(be, KrylovBackend):                  # the method, as Krylov's `backend` names its solver type (src/KKT/Krylov/spd.jl:48)
        name += {"cg": " CG", "minres": " MINRES", "tricg": " TriCG"}[be.method] + (", Jacobi" if be.precond == _lib.PRECOND_JACOBI else "")
    return name


def linear_system(kkt):
    """KKT.linear_system (KKT.jl:121; spd.jl:3)."""
    return _lib.lib().tlpk_linear_system(kkt._h if kkt is not None else None).decode()


def run_ls_tests(A, kkt, atol=SQRT_EPS):
    """The reference's conformance routine for a KKT backend, restated
    (/root/reference/src/KKT/Test/test.jl:9-47): update! with all-ones, solve! with all-ones,
    both residual infinity-norms <= atol.  Returns (rp_norm, rd_norm)."""
    import scipy.sparse as sp
    assert callable(update) and callable(solve)          # test.jl:19-20 hasmethod checks
    Ad = A if sp.issparse(A) or isinstance(kkt, HIPDenseNormalEquations) else sp.csc_matrix(np.asarray(A, dtype=np.float64))
    m, n = Ad.shape
    th = np.ones(n); rp = np.ones(n); rd = np.ones(m)
    update(kkt, th, rp, rd)                              # test.jl:26-29
    xp = np.ones(m); xd = np.ones(n)
    dx = np.zeros(n); dy = np.zeros(m)
    solve(dx, dy, kkt, xp, xd)                           # test.jl:32-36
    r_p = Ad @ dx + rd * dy - xp                         # test.jl:39
    r_d = -dx * (th + rp) + Ad.T @ dy - xd               # test.jl:40
    np_, nd_ = float(np.abs(r_p).max(initial=0.0)), float(np.abs(r_d).max(initial=0.0))
    if not (np_ <= atol and nd_ <= atol):
        raise AssertionError(f"run_ls_tests residuals {np_:.3e}, {nd_:.3e} exceed atol={atol:.3e}")
    return np_, nd_
