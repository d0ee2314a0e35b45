# libtlpk.jl -- ccall shim over the C ABI of libtlpk.so (include/tlpk.h).
#
# Where it goes in Tulip: `src/LinearAlgebra/libtlpk.jl`, included from
# `src/LinearAlgebra/LinearAlgebra.jl` INSIDE `module TLPLinearAlgebra` (reference file:
# /root/reference/src/LinearAlgebra/LinearAlgebra.jl:1-33), i.e. it becomes `Tulip.TLPLinearAlgebra.LibTLPK`;
# src/KKT/HIP/hip.jl reaches it with `using ...TLPLinearAlgebra.LibTLPK`.
# Nothing here touches src/IPM.  No CUDA.jl / AMDGPU.jl: plain `ccall` on a C-ABI shared library.
#
# NOTE: Julia is not available in the build or GPU images of this project, so this file has been
# reviewed by eye against include/tlpk.h but never executed.  It is deliberately mechanical.
module LibTLPK

using Libdl

const libtlpk = Ref{String}(get(ENV, "TULIP_LIBTLPK", "libtlpk.so"))

# The library runs up to 4 HIP streams concurrently; the ROCm runtime multiplexes the process's streams onto
# GPU_MAX_HW_QUEUES hardware queues (4 by default), read at the first HIP call of the process.  A tuning knob of the
# HOST process (the library never touches the environment): set it here unless the user already did.
function __init__()
    haskey(ENV, "GPU_MAX_HW_QUEUES") || (ENV["GPU_MAX_HW_QUEUES"] = "8")
    return nothing
end

const TLPK_SYSTEM_K1 = Int32(0)
const TLPK_SYSTEM_K2 = Int32(1)
const TLPK_KRYLOV_NONE = Int32(0)
const TLPK_KRYLOV_CG = Int32(1)
const TLPK_KRYLOV_MINRES = Int32(16)    # the K2 methods start at 16
const TLPK_KRYLOV_TRICG = Int32(32)     # the quasi-definite K2 methods start at 32 (33 is reserved for TriMR)

# return codes (include/tlpk.h)
const TLPK_OK = Cint(0)
const TLPK_NOT_POSDEF = Cint(1)
const TLPK_BADARG = Cint(2)
const TLPK_OOM = Cint(3)
const TLPK_HIPERR = Cint(4)
const TLPK_NO_DEVICE = Cint(5)
const TLPK_TOO_LARGE = Cint(6)
const TLPK_NOT_FACTORED = Cint(7)

# mirror of `tlpk_options` (field order and types must match include/tlpk.h)
Base.@kwdef mutable struct Options
    struct_size::Int32 = 0
    device::Int32 = 0
    ordering::Int32 = 0          # TLPK_ORDER_AMD
    relax::Int32 = 1
    profile::Int32 = 0
    rank::Int32 = 0
    nranks::Int32 = 1
    streams::Int32 = 0
    user_perm::Ptr{Int64} = C_NULL
    row_block::Ptr{Int64} = C_NULL
    mem_budget_bytes::Int64 = 0
    system::Int32 = 0            # TLPK_SYSTEM_K1 | TLPK_SYSTEM_K2
    refine_steps::Int32 = 0
    detect_blocks::Int32 = 0     # 1: the library finds the block-angular structure of the matrix it is given
    keep_on_too_large::Int32 = 0   # 1: tlpk_create returns a live analyse-only handle with TLPK_TOO_LARGE
    max_link_rows::Int64 = 0
    dense_cols::Int32 = 0        # 1: columns with more than dense_col_min entries (or flagged in col_dense) become augmented nodes (K1)
    max_dense_cols::Int32 = 0    # cap on their number; 0 = 1024
    dense_col_min::Int64 = 0     # 0 = 1000
    col_dense::Ptr{Int64} = C_NULL
    krylov::Int32 = 0            # TLPK_KRYLOV_NONE | TLPK_KRYLOV_CG: matrix-free conjugate gradients on the normal equations (K1) | TLPK_KRYLOV_MINRES: MINRES on K2 | TLPK_KRYLOV_TRICG: TriCG on K2
    krylov_precond::Int32 = 0    # 0 = none | 1 = Jacobi
    krylov_itmax::Int64 = 0      # 0 = 2 m (MINRES, TriCG: 2 (m + n))
    krylov_atol::Float64 = 0.0   # 0 = sqrt(eps)
    krylov_rtol::Float64 = 0.0
end

strerror(code::Integer) = unsafe_string(ccall((:tlpk_strerror, libtlpk[]), Cstring, (Cint,), code))
last_error(h::Ptr{Cvoid}) = unsafe_string(ccall((:tlpk_last_error, libtlpk[]), Cstring, (Ptr{Cvoid},), h))
# a failed tlpk_create / tlpk_create_multi returns no handle: the diagnostic of the calling thread's last failed create
last_create_error() = unsafe_string(ccall((:tlpk_last_create_error, libtlpk[]), Cstring, ()))
backend_name() = unsafe_string(ccall((:tlpk_backend_name, libtlpk[]), Cstring, ()))
system_name() = unsafe_string(ccall((:tlpk_system_name, libtlpk[]), Cstring, ()))
linear_system(h::Ptr{Cvoid}) = unsafe_string(ccall((:tlpk_linear_system, libtlpk[]), Cstring, (Ptr{Cvoid},), h))

"""
    create(A; device, row_block) -> Ptr{Cvoid}

`tlpk_create`: host analyse (ordering, elimination tree, supernodes) + upload.  `A` is passed
with its 1-based `colptr`/`rowval` (index_base = 1); the library copies everything.
"""
function create(m::Int, n::Int, colptr::Vector{Int}, rowval::Vector{Int}, nzval::Vector{Float64};
                device::Integer=0, row_block::Union{Nothing,Vector{Int}}=nothing, system::Int32=TLPK_SYSTEM_K1,
                streams::Integer=0, ngpus::Integer=1, devices::Union{Nothing,Vector{Int32}}=nothing, refine::Integer=0,
                detect_blocks::Bool=false, max_link_rows::Integer=0,
                dense_cols::Union{Nothing,Symbol,Vector{Int}}=nothing, max_dense_cols::Integer=0, dense_col_min::Integer=0)
    opt = Options()
    opt.struct_size = Int32(sizeof(Options))
    opt.device = Int32(device)
    opt.system = system
    opt.streams = Int32(streams)
    opt.refine_steps = Int32(refine)
    opt.detect_blocks = Int32(detect_blocks && row_block === nothing)
    opt.max_link_rows = Int64(max_link_rows)
    # dense_cols: nothing = off, :auto = the count rule, a vector of 1-based column indices = those columns (and the rule)
    opt.dense_cols = Int32(dense_cols !== nothing)
    opt.max_dense_cols = Int32(max_dense_cols)
    opt.dense_col_min = Int64(dense_col_min)
    cd = zeros(Int64, dense_cols isa Vector{Int} ? n : 0)
    dense_cols isa Vector{Int} && (cd[dense_cols] .= 1)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rb = row_block === nothing ? Int[] : row_block
    dv = devices === nothing ? Int32[] : devices
    rc = GC.@preserve colptr rowval nzval rb dv cd opt begin
        row_block === nothing || (opt.row_block = pointer(rb))
        dense_cols isa Vector{Int} && (opt.col_dense = pointer(cd))
        if ngpus > 1
            # one Julia process, several GPUs: block-angular LPs only (tlpk_create_multi, include/tlpk.h)
            ccall((:tlpk_create_multi, libtlpk[]), Cint,
                  (Ref{Ptr{Cvoid}}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Cint, Ref{Options}, Cint, Ptr{Int32}),
                  h, m, n, colptr, rowval, nzval, 1, opt, ngpus, devices === nothing ? Ptr{Int32}(C_NULL) : pointer(dv))
        else
            ccall((:tlpk_create, libtlpk[]), Cint,
                  (Ref{Ptr{Cvoid}}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Cint, Ref{Options}),
                  h, m, n, colptr, rowval, nzval, 1, opt)
        end
    end
    return rc, h[]
end

"""
    create_dense(A; device, profile, mem_budget_bytes) -> (rc, Ptr{Cvoid})

`tlpk_create_dense`: a dense column-major `Matrix{Float64}` (leading dimension = its number of rows); K1 only, one GPU.  The
library copies `A` to the device; nothing is retained.
"""
function create_dense(A::Matrix{Float64}; device::Integer=0, profile::Bool=false, mem_budget_bytes::Integer=0)
    m, n = size(A)
    opt = Options()
    opt.struct_size = Int32(sizeof(Options))
    opt.device = Int32(device)
    opt.profile = Int32(profile)
    opt.mem_budget_bytes = Int64(mem_budget_bytes)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve A opt ccall((:tlpk_create_dense, libtlpk[]), Cint,
        (Ref{Ptr{Cvoid}}, Int64, Int64, Ptr{Float64}, Int64, Ref{Options}),
        h, m, n, A, max(m, 1), opt)
    return rc, h[]
end

"""
    create_krylov(m, n, colptr, rowval, nzval; device, precond, itmax, atol, rtol, profile, mem_budget_bytes, method) -> (rc, Ptr{Cvoid})

`tlpk_create` with `krylov = TLPK_KRYLOV_CG`: no analysis, no factor; every solve runs conjugate gradients on the device.
`precond`: `:none` or `:jacobi`.  `method = :minres`: `krylov = TLPK_KRYLOV_MINRES` and `system = TLPK_SYSTEM_K2`, MINRES on the
augmented system.  `method = :tricg`: `krylov = TLPK_KRYLOV_TRICG` and `system = TLPK_SYSTEM_K2`, TriCG on its quasi-definite form;
`precond` must be `:none`.
"""
function create_krylov(m::Int, n::Int, colptr::Vector{Int}, rowval::Vector{Int}, nzval::Vector{Float64};
                       device::Integer=0, precond::Symbol=:none, itmax::Integer=0, atol::Real=0.0, rtol::Real=0.0,
                       profile::Bool=false, mem_budget_bytes::Integer=0, method::Symbol=:cg)
    method in (:cg, :minres, :tricg) || throw(ArgumentError("method: :cg, :minres or :tricg"))
    opt = Options()
    opt.struct_size = Int32(sizeof(Options))
    opt.device = Int32(device)
    opt.profile = Int32(profile)
    opt.mem_budget_bytes = Int64(mem_budget_bytes)
    opt.krylov = method === :tricg ? TLPK_KRYLOV_TRICG : method === :minres ? TLPK_KRYLOV_MINRES : TLPK_KRYLOV_CG
    opt.system = method === :cg ? TLPK_SYSTEM_K1 : TLPK_SYSTEM_K2
    opt.krylov_precond = Int32(precond === :jacobi)
    opt.krylov_itmax = Int64(itmax)
    opt.krylov_atol = Float64(atol)
    opt.krylov_rtol = Float64(rtol)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    rc = GC.@preserve colptr rowval nzval opt ccall((:tlpk_create, libtlpk[]), Cint,
        (Ref{Ptr{Cvoid}}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Cint, Ref{Options}),
        h, m, n, colptr, rowval, nzval, 1, opt)
    return rc, h[]
end

destroy(h::Ptr{Cvoid}) = ccall((:tlpk_destroy, libtlpk[]), Cvoid, (Ptr{Cvoid},), h)

"""
    detect_blocks(m, n, colptr, rowval; max_link_rows=0) -> (row_block::Vector{Int}, n_blocks, n_link)

`tlpk_detect_blocks`: block id (0-based, -1 = linking row) of every row of a 1-based CSC matrix; `n_blocks == 1` means
no block-angular structure was found.
"""
function detect_blocks(m::Int, n::Int, colptr::Vector{Int}, rowval::Vector{Int}; max_link_rows::Integer=0)
    rb = zeros(Int, max(m, 1)); nb = Ref{Int64}(1); nl = Ref{Int64}(0)
    rc = GC.@preserve colptr rowval rb ccall((:tlpk_detect_blocks, libtlpk[]), Cint,
        (Int64, Int64, Ptr{Int64}, Ptr{Int64}, Cint, Int64, Ptr{Int64}, Ref{Int64}, Ref{Int64}),
        m, n, colptr, rowval, 1, max_link_rows, rb, nb, nl)
    rc == TLPK_OK || error("tlpk_detect_blocks: " * strerror(rc))
    return resize!(rb, m), Int(nb[]), Int(nl[])
end

"""
    set_values!(h, nzval) / set_values!(h, A::Matrix{Float64})

`tlpk_set_values` / `tlpk_set_values_dense`: new numerical values on the pattern the handle was analysed on (`nzval` in the order of
the `SparseMatrixCSC` given to `create`).  The analysis is kept; the handle is not factored afterwards.
"""
set_values!(h::Ptr{Cvoid}, nzval::Vector{Float64}) =
    GC.@preserve nzval ccall((:tlpk_set_values, libtlpk[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), h, nzval, length(nzval))
set_values!(h::Ptr{Cvoid}, A::Matrix{Float64}) =
    GC.@preserve A ccall((:tlpk_set_values_dense, libtlpk[]), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), h, A, max(size(A, 1), 1))

"""
    ipm_reload!(h; b, c, l, u)

`tlpk_ipm_reload`: new LP data for the device-resident loops of a handle that has been loaded (`nothing` = keep the vector).
"""
function ipm_reload!(h::Ptr{Cvoid}; b::Union{Nothing,Vector{Float64}}=nothing, c::Union{Nothing,Vector{Float64}}=nothing,
                     l::Union{Nothing,Vector{Float64}}=nothing, u::Union{Nothing,Vector{Float64}}=nothing)
    p(v) = v === nothing ? Ptr{Float64}(C_NULL) : pointer(v)
    return GC.@preserve b c l u ccall((:tlpk_ipm_reload, libtlpk[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, p(b), p(c), p(l), p(u))
end

# tlpk_ipm_get(h, what, host, len) reads one device vector of a loaded handle (read-only; `len` = its length):
#   what 0-5 x, xl, xu, zl, zu (n), y (m) | 6-11 accepted direction | 12-17 candidate direction (same order) | 18-21 rp (m), rl, ru, rd
#   | 22-26 thl, thu, hx, hy (m), hxid | 27-32 xil, xiu, xzl, xzu, xid, xip (m) | 33-35 theta_inv, regP (n), regD (m) of the last factor call.
#   Codes above 5: single-device handles only (TLPK_BADARG on a multi-device one).
ipm_get!(h::Ptr{Cvoid}, what::Integer, host::Vector{Float64}) =
    GC.@preserve host ccall((:tlpk_ipm_get, libtlpk[]), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Int64), h, what, host, length(host))

# Block skip (include/tlpk.h): skip[k] != 0 leaves block k of `row_block` out of the following update! / solve! calls; `nothing` lifts the mask.
block_skip!(h::Ptr{Cvoid}, skip::Vector{UInt8}) =
    GC.@preserve skip ccall((:tlpk_block_skip, libtlpk[]), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int64), h, skip, length(skip))
block_skip!(h::Ptr{Cvoid}, ::Nothing, nblocks::Integer) =
    ccall((:tlpk_block_skip, libtlpk[]), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int64), h, C_NULL, nblocks)
# batch-loaded handles: the tlpk_ipm_batch_* / tlpk_mpc_batch_* calls leave the parked LPs' blocks out of their update and solves
ipm_batch_skip!(h::Ptr{Cvoid}, on::Bool) = ccall((:tlpk_ipm_batch_skip, libtlpk[]), Cint, (Ptr{Cvoid}, Cint), h, on ? 1 : 0)

update(h::Ptr{Cvoid}, θinv::Vector{Float64}, regP::Vector{Float64}, regD::Vector{Float64}) =
    GC.@preserve θinv regP regD ccall((:tlpk_update, libtlpk[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, θinv, regP, regD)

solve(h::Ptr{Cvoid}, dx::Vector{Float64}, dy::Vector{Float64}, ξp::Vector{Float64}, ξd::Vector{Float64}) =
    GC.@preserve dx dy ξp ξd ccall((:tlpk_solve, libtlpk[]), Cint,
        (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, dx, dy, ξp, ξd)

end  # module
