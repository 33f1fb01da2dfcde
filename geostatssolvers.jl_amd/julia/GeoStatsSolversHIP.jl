# GeoStatsSolversHIP.jl -- Julia host shim over libgss_hip.so (include/gss.h).
#
# Drop-in for the KrigingSolver / FFTGS / LUGS methods of juliohm/GeoStatsSolvers.jl v0.7.16:
# the solver types keep the reference's parameter surface (src/estimation/krig.jl:64-74,
# src/simulation/fft.jl:51-60, src/simulation/lu.jl:67-74) and extend the same GeoStatsBase
# generics (`solve`, `preprocess`, `solvesingle`, src/GeoStatsSolvers.jl:28); the arithmetic the
# reference delegates to Variography / GeoStatsModels / FFTW / LinearAlgebra is replaced by `ccall`s.
#
# NOTE: there is no Julia toolchain in the build environment, so this file has never been executed;
# the executable twin with identical logic is geostatssolvers.jl_amd/gss/solvers.py, which the test
# suite drives through the same C-ABI (tests/test_generic_loop.py replays GeoStatsBase's call sequence against
# it).  Keep the two in step.
#
# Realisation indices.  GeoStatsBase's loop calls `solvesingle(problem, covars, solver, preproc)` with four
# positional arguments and no realisation index (test/dummy.jl:22; fft.jl:145, lu.jl:171, seq.jl:76), while the
# device noise is keyed on (seed, realisation).  `preprocess` therefore draws the seed from `solver.rng` once
# (the reference consumes the same rng, fft.jl:147 / lu.jl:173) and creates one atomic call counter per
# covariable group; the k-th `solvesingle` call of a group produces realisation k - 1.  `solve` is also
# specialised for the three simulation solvers: it produces all realisations of a variable in ONE device call
# (same indices, same fields) and frees the device state before returning.
# Several GPUs: `solve(problem, solver; procs=workers())` with ONE worker process per GPU (Distributed), each bound to its
# device by `GeoStatsSolversHIP.bind_device(dev)`.  The first worker runs the preprocess (fft.jl:62, lu.jl:76 -- once, as
# the reference), exports an 80-byte HIP-IPC token per device state, the other workers create their handles without state
# and pull it over their own xGMI link (gss_state_ipc_import); every worker then realises a contiguous block of
# realisations -- realisation r depends on (seed, r) only, so the ensemble equals the single-process one.  Kriging shards
# the domain the same way (the factor is recomputed per worker: cheaper than moving it below a few thousand data).
module GeoStatsSolversHIP

using Meshes
using GeoTables
using Variography
using GeoStatsBase
using Tables
using Random
using Unitful
using LinearAlgebra: cholesky, lu      # values of LUGS' `factorization` parameter (lu.jl:70)
using LinearAlgebra: Symmetric, det, eigen   # principal axes of a ball's metric (ballrotmatrix)
using Distances: evaluate              # the search metric applied to a pair of points (closure weights of LWR)
using CoDa: Composition, components    # compositional value columns (test/estimation/idw.jl:47-65); [RECALL] accessor names
using Distributed: myid, remotecall_fetch

import GeoStatsBase: solve, preprocess, solvesingle

export KrigingSolverHIP, IDWSolverHIP, LWRSolverHIP, ExpWeight, TricubeWeight, FFTGSHIP, LUGSHIP, SGSHIP
export krig_fit, krig_predict_device!, fftgs_realize_device!, bind_device
export empirical_variogram, fit_variogram, empirical_varioplane, fit_anisotropic
export empirical_cross_variogram, fit_lmc, pairindex
export cverror, krig_cv_global, cv_summary, CVSummary

const libgss = get(ENV, "LIBGSS_HIP", "libgss_hip.so")

const GSS_MEM_HOST = Int32(0)
const GSS_MEM_DEVICE = Int32(1)
const GSS_FFTGS_NO_SPECTRUM = Int32(1)
const GSS_LUGS_NO_FACTOR = Int32(1)
const GSS_STATE_FFTGS = Int32(1)
const GSS_STATE_LUGS = Int32(2)
const GSS_IPC_TOKEN_BYTES = 96
const GSS_KRIG_NO_FACTOR = Int32(1)
const GSS_KRIG_ASYNC_FIT = Int32(2)     # fit beside the first assembly; status at the first global prediction
const GSS_LUGS_FACT_LU = Int32(2)
const GSS_SGS_MASK_AFTER_SEARCH = Int32(1)
const GSS_SGS_METRIC_SHIFT = 4

# ---- units (src/utils.jl:5-15): affine units are made absolute before the values are stripped for the device;
#      estimates get the unit back, variances its square (krig.jl:94,160; idw.jl:109; lwr.jl:112,153) --------------
elunit(x) = typeunit(nonmissingtype(eltype(x)))
typeunit(::Type) = NoUnits
typeunit(::Type{Q}) where {Q<:Quantity} = unit(Q)
uadjust(x) = uadjust(elunit(x), x)
uadjust(::Unitful.Units, x) = x
uadjust(U::Unitful.AffineUnits, x) = map(v -> ismissing(v) ? missing : uconvert(absoluteunit(U), v), x)
# (stripped Float64 values of the non-missing entries, unit to re-attach)
function stripunits(vals)
  z = uadjust(vals)
  Float64.(ustrip.(collect(skipmissing(z)))), elunit(z)
end

# ---- device handles: owned by the library, destroyed by a finalizer (or explicitly at the end of `solve`) -------
mutable struct Handle
  ptr::Ptr{Cvoid}
  kind::Symbol                     # :krig, :fftgs, :lugs, :sgs
  function Handle(ptr, kind)
    h = new(ptr, kind)
    finalizer(destroy!, h)
    h
  end
end
function destroy!(h::Handle)
  h.ptr == C_NULL && return nothing
  if h.kind === :fftgs
    ccall((:gss_fftgs_destroy, libgss), Int32, (Ptr{Cvoid},), h.ptr)
  elseif h.kind === :lugs
    ccall((:gss_lugs_destroy, libgss), Int32, (Ptr{Cvoid},), h.ptr)
  elseif h.kind === :sgs
    ccall((:gss_sgs_destroy, libgss), Int32, (Ptr{Cvoid},), h.ptr)
  else
    ccall((:gss_krig_destroy, libgss), Int32, (Ptr{Cvoid},), h.ptr)
  end
  h.ptr = C_NULL
  nothing
end
Base.unsafe_convert(::Type{Ptr{Cvoid}}, h::Handle) = h.ptr

# ---- realisation bookkeeping (see the header) ---------------------------------------------------------------------
struct RunState
  seed::UInt64
  next::Dict{Any,Threads.Atomic{Int}}     # covars.names => number of solvesingle calls so far
  vindex::Dict{Symbol,Int}                # variable => 0-based position among variables(problem)
  owner::Int                              # process that owns the device handles
end
function RunState(problem, solver; seed=nothing)
  allcovars = covariables(problem, solver)
  RunState(isnothing(seed) ? rand(solver.rng, UInt64) : UInt64(seed), Dict{Any,Threads.Atomic{Int}}(c.names => Threads.Atomic{Int}(0) for c in allcovars),
           Dict{Symbol,Int}(v => i - 1 for (i, v) in enumerate(keys(variables(problem)))), myid())
end
function nextreal!(run::RunState, conames)
  run.owner == myid() || error("the device state of this preprocess lives in process $(run.owner); use procs=[myid()]")
  Threads.atomic_add!(run.next[conames], 1)       # returns the value before the increment
end
varseed(run::RunState, var) = run.seed + UInt64(run.vindex[var])

# ---- C structs ---------------------------------------------------------------------------
struct GssVgExtra              # one additional nested structure of gss_variogram_t
  kind::Int32
  aniso::Int32
  sill::Float64
  range::Float64
  nu::Float64
  inv_radii::NTuple{3,Float64}
end

struct GssVariogram            # gss_variogram_t
  kind::Int32
  dim::Int32
  sill::Float64
  nugget::Float64
  range::Float64
  nu::Float64
  aniso::Int32
  reserved::Int32
  inv_radii::NTuple{3,Float64}
  nextra::Int32
  reserved2::Int32
  extra::NTuple{3,GssVgExtra}
  rotation::NTuple{9,Float64}  # row-major 3 x 3, read where a structure has aniso = 2
end

const NOEXTRA = GssVgExtra(Int32(0), Int32(0), 0.0, 1.0, 1.0, (1.0, 1.0, 1.0))
const NOROT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
const GSS_METRIC_ROTATED_BALL = Int32(4)

# Rotation of a ball as the row-major 3 x 3 of gss_variogram_t (identity on absent axes), or `nothing` for an
# isotropic ball or the identity.  Convention (gss.h): principal axes in the columns of R, d(x, y) =
# ||diag(1/r) R' (x - y)||, M = R diag(r^-2) R'.  [RECALL] Meshes' `rotation(ball)` accessor; if the loaded Meshes
# differs, derive R and r from `metric(ball).qmat` by `eigen(Symmetric(Q))` (INTEGRATION.md).
function ballrotation(ball)
  rs = radii(ball)
  d = length(rs)
  (d == 1 || allequal(rs)) && return nothing        # a sphere: every rotation describes the same ball
  R = Matrix{Float64}(ballrotmatrix(ball))
  size(R) == (d, d) || throw(ArgumentError("rotation of a $d-D ball must be $d x $d"))
  all(R[i, j] == (i == j ? 1.0 : 0.0) for i in 1:d, j in 1:d) && return nothing
  ntuple(k -> (i = (k - 1) ÷ 3 + 1; j = (k - 1) % 3 + 1; i <= d && j <= d ? R[i, j] : Float64(i == j)), 9)
end

# R of a ball: the `rotation` accessor where the loaded Meshes has one, otherwise the principal axes of its metric
# (Q = R diag(r^-2) R', columns ordered as the radii, det R = +1)
function ballrotmatrix(ball)
  isdefined(Meshes, :rotation) && hasmethod(Meshes.rotation, Tuple{typeof(ball)}) && return Meshes.rotation(ball)
  Q = Matrix{Float64}(metric(ball).qmat)
  F = eigen(Symmetric(Q))
  r = ustrip.(radii(ball))
  R = zeros(length(r), length(r))
  used = falses(length(r))
  for j in eachindex(r)          # the eigenvector whose eigenvalue is r_j^-2
    i = argmin([used[k] ? Inf : abs(F.values[k] - 1 / r[j]^2) for k in eachindex(r)])
    used[i] = true
    R[:, j] = F.vectors[:, i]
  end
  det(R) < 0 && (R[:, end] .*= -1)
  R
end

function check(code::Int32)
  code == 0 && return nothing
  buf = Vector{UInt8}(undef, 512)
  ccall((:gss_last_error, libgss), Int32, (Ptr{UInt8}, Int32), buf, 512)
  msg = unsafe_string(pointer(buf))
  code == 1 && throw(ArgumentError(msg))          # GSS_ERR_INVALID (krig.jl:100-102, fft.jl:91-93)
  code == 3 && throw(ErrorException("not positive definite: " * msg))
  error("libgss_hip error $code: $msg")
end

vgkind(::GaussianVariogram) = Int32(0)
vgkind(::ExponentialVariogram) = Int32(1)
vgkind(::SphericalVariogram) = Int32(2)
vgkind(::MaternVariogram) = Int32(3)
vgkind(::CubicVariogram) = Int32(4)
vgkind(::PentasphericalVariogram) = Int32(5)
vgkind(::SineHoleVariogram) = Int32(6)

# The nugget the loaded Variography evaluates with.  [RECALL] its `GaussianVariogram` functor adds a small constant
# ("add small eps to nugget for numerical stability": `n = nugget + 1e-6`) that the `nugget(γ)` accessor does not
# show -- the reason the reference's suite can factor Gaussian covariances of 10^4 cells with nugget 0
# (test/simulation/lu.jl:29-64).  The parameters cross the C-ABI, not the functor, so the rule is applied here;
# `GeoStatsSolversHIP.GAUSSIAN_NUGGET_EPS[] = 0.0` switches it off.
const GAUSSIAN_NUGGET_EPS = Ref(1e-6)
effnugget(γ) = Float64(ustrip(nugget(γ)))
effnugget(γ::GaussianVariogram) = Float64(ustrip(nugget(γ))) + GAUSSIAN_NUGGET_EPS[]
effnugget(γ::NestedVariogram) = sum(Float64(c) * effnugget(g) for (c, g) in zip(γ.cs, γ.γs))

function structure(γ)            # (kind, aniso, range, nu, inv_radii, rotation or nothing) of one basic model
  ball = metricball(γ)
  rs = radii(ball)
  aniso = length(rs) > 1
  ir = ntuple(i -> aniso && i <= length(rs) ? 1.0 / ustrip(rs[i]) : 1.0, 3)
  ν = γ isa MaternVariogram ? Float64(γ.order) : 1.0
  rot = aniso ? ballrotation(ball) : nothing
  (vgkind(γ), Int32(isnothing(rot) ? aniso : 2), aniso ? 1.0 : Float64(ustrip(range(γ))), ν, ir, rot)
end

# `extent` = diameter of the data bounding box: only needed for the non-stationary PowerVariogram, which the
# device handles through the pseudo-covariance A - gamma(h) with A = 2 gamma(extent) (gss.h, GSS_VG_POWER);
# the kriging solver passes it, the simulation solvers do not and therefore keep the reference's assertion.
function cvariogram(γ, dim; extent=nothing)
  if γ isa PowerVariogram && !isnothing(extent)
    A = 2 * Float64(γ.scaling) * Float64(extent)^Float64(γ.exponent) + Float64(nugget(γ)) + floatmin(Float64)
    return GssVariogram(Int32(7), Int32(dim), A, Float64(nugget(γ)), Float64(γ.scaling), Float64(γ.exponent), Int32(0),
                        Int32(0), (1.0, 1.0, 1.0), Int32(0), Int32(0), (NOEXTRA, NOEXTRA, NOEXTRA), NOROT)
  end
  isstationary(γ) || throw(ArgumentError("variogram model must be stationary"))   # fft.jl:91-93, lu.jl:110
  if γ isa NestedVariogram       # gamma = sum c_i gamma_i: first structure carries the total nugget
    cs, γs = γ.cs, γ.γs
    for g in γs      # a structure whose (regularised) nugget exceeds its sill has a negative structured part: refused, not dropped
      effnugget(g) <= Float64(ustrip(sill(g))) ||
        throw(ArgumentError("nested variogram: the (regularised) nugget of a structure exceeds its sill"))
    end
    keep = [i for i in eachindex(γs) if cs[i] * (sill(γs[i]) - effnugget(γs[i])) > 0]
    length(keep) <= 4 || throw(ArgumentError("at most 4 nested structures are supported on the device"))
    k0, a0, r0, ν0, ir0, rot0 = structure(γs[keep[1]])
    # one rotation for every rotated structure (gss.h); different rotations per structure are not supported
    # anisotropic structures share one rotation; an axis-aligned one (aniso = 1) counts as the identity
    aniso_rots = [structure(γs[i])[6] for i in keep if structure(γs[i])[2] != 0 && !allequal(structure(γs[i])[5][1:dim])]
    rots = unique([r for r in aniso_rots if !isnothing(r)])
    (isempty(rots) || (length(rots) == 1 && !any(isnothing, aniso_rots))) ||
      throw(ArgumentError("nested variogram: the anisotropic structures have different rotations (an axis-aligned " *
                          "ball counts as the identity); all anisotropic structures of one model must share one rotation"))
    nug = effnugget(γ)
    extras = ntuple(3) do j
      j + 1 > length(keep) && return NOEXTRA
      i = keep[j+1]
      k, a, r, ν, ir, _ = structure(γs[i])
      GssVgExtra(k, a, Float64(cs[i] * (sill(γs[i]) - effnugget(γs[i]))), r, ν, ir)
    end
    c0 = Float64(cs[keep[1]] * (sill(γs[keep[1]]) - effnugget(γs[keep[1]])))
    return GssVariogram(k0, Int32(dim), c0 + nug, nug, r0, ν0, a0, Int32(0), ir0, Int32(length(keep) - 1), Int32(0), extras,
                        isempty(rots) ? NOROT : rots[1])
  end
  k, a, r, ν, ir, rot = structure(γ)
  GssVariogram(k, Int32(dim), Float64(sill(γ)), effnugget(γ), r, ν, a, Int32(0), ir, Int32(0), Int32(0),
               (NOEXTRA, NOEXTRA, NOEXTRA), isnothing(rot) ? NOROT : rot)
end

# solver parameter `distance` (krig.jl:72, idw.jl:54, lwr.jl:57) -> (GSS_METRIC_*, parameter); a neighbourhood
# overrides it exactly as searcher_ui does (ui.jl:25-31)
metricspec(::Euclidean) = (Int32(0), 0.0)
metricspec(::Cityblock) = (Int32(1), 0.0)
metricspec(::Chebyshev) = (Int32(2), 0.0)
metricspec(d::Haversine) = (Int32(3), Float64(d.radius))
metricspec(d) = throw(ArgumentError("search distance $d is not available on the device"))
searchmetric(p) = isnothing(p.neighborhood) ? metricspec(p.distance) :
                  (isnothing(ballrotation(p.neighborhood)) ? Int32(0) : GSS_METRIC_ROTATED_BALL, 0.0)

# Point-major coordinates: a d x n Julia matrix is already in the layout the C-ABI wants.  Three methods, because for
# 10^6 - 10^7 elements the generic one -- a `centroid` call and a small vector per element -- would be the `solve` time:
#   * CartesianGrid: the centroids are origin + (index - 1/2) * spacing per axis, first axis fastest (the order of the
#     grid's elements and of every realisation vector): d ranges and one pass over the matrix, nothing per element;
#   * PointSet of Float64 points: the coordinate vectors ARE the columns -- one `reinterpret`, no copy of the data
#     beyond the final `Matrix` (the C side wants contiguous memory that stays put during the call);
#   * views of either (`view(domain, inds)`, `parentindices`): the parent's matrix, then the selected columns;
#   * anything else: element by element.
function coordmatrix(g::CartesianGrid)
  dims = size(g)
  d = length(dims)
  o = Float64[ustrip.(coordinates(minimum(g)))...]
  sp = Float64[ustrip.(spacing(g))...]
  axes = [o[a] .+ ((1:dims[a]) .- 0.5) .* sp[a] for a in 1:d]
  X = Matrix{Float64}(undef, d, prod(dims))
  j = 0
  for I in CartesianIndices(dims)          # first index fastest = the linear order of the grid's elements
    j += 1
    for a in 1:d
      X[a, j] = axes[a][I[a]]
    end
  end
  X
end
function coordmatrix(ps::PointSet)
  n = nelements(ps)
  n == 0 && return Matrix{Float64}(undef, embeddim(ps), 0)
  v = [ustrip.(coordinates(ps[i])) for i in 1:n]                  # Vector of static coordinate vectors
  eltype(eltype(v)) === Float64 ? Matrix(reinterpret(reshape, Float64, v)) : Float64.(reduce(hcat, v))
end
function coordmatrix(dom)
  if parent(dom) !== dom && (parent(dom) isa CartesianGrid || parent(dom) isa PointSet)
    return coordmatrix(parent(dom))[:, collect(parentindices(dom))]
  end
  reduce(hcat, [collect(Float64, ustrip.(coordinates(centroid(dom, i)))) for i in 1:nelements(dom)])
end

# ---- KrigingSolver ------------------------------------------------------------------------
@estimsolver KrigingSolverHIP begin
  @param variogram = GaussianVariogram()
  @param mean = nothing
  @param degree = nothing
  @param drifts = nothing
  @param minneighbors = 1
  @param maxneighbors = nothing
  @param neighborhood = nothing
  @param distance = Euclidean()
  @param path = LinearPath()
  # not a parameter of the reference (krig.jl:180 always hands the cell of a grid to predictprob, whose dependencies
  # regularise over it): :point estimates at the centroids; (:block, nsub) regularises over the cells of a Cartesian grid
  # by the midpoint rule with nsub points per axis (gss_krig_set_block_support)
  @param support = :point
end

# `procs`: one worker per GPU, each estimates a contiguous block of the domain (krig.jl:180,205: the points are
# independent given the data; the factor is recomputed per worker) -- see solve_points_on_workers below
function solve(problem::EstimationProblem, solver::KrigingSolverHIP; procs=[myid()])
  procs == [myid()] || return solve_points_on_workers(problem, solver, collect(procs))
  pdata = data(problem)
  pdomain = domain(problem)
  dtable = values(pdata)
  ddomain = domain(pdata)
  X0 = coordmatrix(pdomain)
  d, m = size(X0)
  μs, σs = [], []
  for covars in covariables(problem, solver), var in covars.names
    p = covars.params[Set([var])]
    zcol = Tables.getcolumn(Tables.columns(dtable), var)
    inds = findall(!ismissing, zcol)                                     # krig.jl:97
    isempty(inds) && throw(AssertionError("all samples of $var are missing, aborting..."))
    z, u = stripunits(zcol)                                              # uadjust, krig.jl:94
    X = coordmatrix(view(ddomain, inds))
    n = length(z)
    # kriging_ui, ui.jl:40-50
    variant, degree, ndrift, Fd, F0 = Int32(1), Int32(0), Int32(0), C_NULL, C_NULL
    skmean = 0.0
    if !isnothing(p.drifts)
      variant, ndrift = Int32(3), Int32(length(p.drifts))
      Fd = Float64[f(Point(X[:, i]...)) for f in p.drifts, i in 1:n]     # ndrift x n == n x ndrift row-major
      F0 = Float64[f(Point(X0[:, i]...)) for f in p.drifts, i in 1:m]
    elseif !isnothing(p.degree)
      variant, degree = Int32(2), Int32(p.degree)
    elseif !isnothing(p.mean)
      variant, skmean = Int32(0), (p.mean isa Quantity ? Float64(ustrip(u, p.mean)) : Float64(p.mean))
    end
    # searcher_ui, ui.jl:11-32
    exact = isnothing(p.maxneighbors)
    k = exact ? n : p.maxneighbors
    if !exact && (k < 1 || k > n)
      @warn "Invalid maximum number of neighbors. Adjusting to $n..."
      k = n
    end
    extent = sqrt(sum(abs2, maximum(X, dims=2) .- minimum(X, dims=2)))
    vg = Ref(cvariogram(p.variogram, d; extent))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    μ = Vector{Float64}(undef, m); σ² = similar(μ); status = Vector{UInt8}(undef, m)
    GC.@preserve X z X0 Fd F0 μ σ² status begin
      check(ccall((:gss_krig_create, libgss), Int32,
                  (Ptr{Ptr{Cvoid}}, Ptr{GssVariogram}, Int32, Float64, Int32, Int32, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Int64, Int32, Ptr{Cvoid}),
                  h, vg, variant, skmean, degree, ndrift, X, z, Fd, n, exact ? GSS_KRIG_ASYNC_FIT : GSS_KRIG_NO_FACTOR, C_NULL))
      try
        if p.support !== :point
          pgrid = parent(pdomain)
          pgrid isa CartesianGrid || throw(ArgumentError("support = :block needs a Cartesian grid domain"))
          cell = Float64[ustrip.(spacing(pgrid))...]
          nsub = p.support === :block ? Int32(3) : Int32(p.support[2])
          GC.@preserve cell check(ccall((:gss_krig_set_block_support, libgss), Int32,
                                        (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Cvoid}), h[], cell, nsub, C_NULL))
        end
        if exact                                                         # krig.jl:166-186
          check(ccall((:gss_krig_predict_global, libgss), Int32,
                      (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Int32,
                       Ptr{Cvoid}), h[], X0, F0, m, μ, σ², status, GSS_MEM_HOST, C_NULL))
        else                                                             # krig.jl:188-234
          radius, ir = ballspec(p.neighborhood)
          met, mpar = searchmetric(p)
          check(ccall((:gss_krig_predict_knn, libgss), Int32,
                      (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Int32, Int32, Float64, Ptr{Float64}, Int32,
                       Float64, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Cvoid}),
                      h[], X0, F0, m, Int32(k), Int32(p.minneighbors), radius, ir, met, mpar, μ, σ², status, C_NULL,
                      C_NULL, GSS_MEM_HOST, C_NULL))
        end
      finally
        ccall((:gss_krig_destroy, libgss), Int32, (Ptr{Cvoid},), h[])
      end
    end
    miss = status .!= 0                                                  # krig.jl:213-214
    inds = collect(traverse(pdomain, p.path))                            # results in traversal order, krig.jl:179-183
    push!(μs, var => [miss[i] ? missing : μ[i] * u for i in inds])
    push!(σs, Symbol(var, "_variance") => [miss[i] ? missing : σ²[i] * u^2 for i in inds])   # krig.jl:160
  end
  georef((; μs..., σs...), pdomain)                                      # krig.jl:163
end

# ---- IDWSolver / LWRSolver (idw.jl:49-153, lwr.jl:53-158) -------------------------------------
struct ExpWeight                 # h -> exp(-a h^p); ExpWeight(3, 2) is the reference default (lwr.jl:58)
  a::Float64
  p::Float64
end
struct TricubeWeight end         # h -> (1 - h^3)^3
(w::ExpWeight)(h) = exp(-w.a * h^w.p)
(::TricubeWeight)(h) = (1 - h^3)^3
weightspec(w::ExpWeight) = (Int32(0), w.a, w.p)
weightspec(::TricubeWeight) = (Int32(1), 0.0, 0.0)
weightspec(f) = throw(ArgumentError("weightfun of this kind is evaluated on the host (lwr_with_closure)"))

@estimsolver IDWSolverHIP begin
  @param minneighbors = 1
  @param maxneighbors = nothing
  @param neighborhood = nothing
  @param distance = Euclidean()
  @param exponent = 1
  @param path = LinearPath()
end

@estimsolver LWRSolverHIP begin
  @param minneighbors = 1
  @param maxneighbors = nothing
  @param neighborhood = nothing
  @param distance = Euclidean()
  @param weightfun = ExpWeight(3.0, 2.0)
  @param path = LinearPath()
end

function neighbor_estimate(problem, solver, auxname, auxunit, call, callcols)
  pdata = data(problem)
  pdomain = domain(problem)
  dtable = values(pdata)
  X0 = coordmatrix(pdomain)
  d, m = size(X0)
  μs, σs = [], []
  for covars in covariables(problem, solver), var in covars.names
    p = covars.params[Set([var])]
    zcol = Tables.getcolumn(Tables.columns(dtable), var)
    inds = findall(!ismissing, zcol)                                     # idw.jl:77, lwr.jl:80
    n = length(inds)
    @assert n > 0 "estimation requires data"
    iscomp = nonmissingtype(eltype(zcol)) <: Composition
    z, u = iscomp ? (Float64[], NoUnits) : stripunits(zcol)              # uadjust, idw.jl:109, lwr.jl:112
    X = coordmatrix(view(domain(pdata), inds))
    nmax = isnothing(p.maxneighbors) ? n : min(p.maxneighbors, n)        # idw.jl:93
    @assert p.minneighbors ≤ nmax "invalid min/max number of neighbors"
    k = nmax
    if !isnothing(p.maxneighbors) && (p.maxneighbors < 1 || p.maxneighbors > n)   # searcher_ui, ui.jl:18-20
      @warn "Invalid maximum number of neighbors. Adjusting to $n..."
      k = n
    end
    radius, ir = ballspec(p.neighborhood)
    aux = Vector{Float64}(undef, m); status = Vector{UInt8}(undef, m)
    if iscomp
      # compositional data (test/estimation/idw.jl:47-65): the loop is generic over the value type -- idw.jl:138
      # `sum(ws[i] * vs[i])` is a perturbation of powers -- and both operations are linear in the log-parts, which travel
      # as value columns of ONE call: one search and one weight vector per estimation point (gss_*_predict_cols)
      L = log.(permutedims(reduce(hcat, [collect(Float64, components(zcol[i])) for i in inds])))   # n x D, a part per column
      D = size(L, 2)
      M = Matrix{Float64}(undef, m, D)
      GC.@preserve X L X0 ir M aux status check(callcols(p, X, L, n, d, Int32(D), X0, m, Int32(k), radius, ir, M, aux, status))
      miss = status .!= 0
      tinds = collect(traverse(pdomain, p.path))
      push!(μs, var => [miss[i] ? missing : Composition(exp.(view(M, i, :))...) for i in tinds])
      push!(σs, Symbol(var, auxname) => [miss[i] ? missing : aux[i] for i in tinds])
      continue
    end
    μ = Vector{Float64}(undef, m)
    GC.@preserve X z X0 ir μ aux status check(call(p, X, z, n, d, X0, m, Int32(k), radius, ir, μ, aux, status))
    miss = status .!= 0                                                  # idw.jl:123-124
    inds = collect(traverse(pdomain, p.path))                            # results in traversal order, idw.jl:112-113
    push!(μs, var => [miss[i] ? missing : μ[i] * u for i in inds])
    push!(σs, Symbol(var, auxname) => [miss[i] ? missing : aux[i] * auxunit(u) for i in inds])
  end
  georef((; μs..., σs...), pdomain)
end

solve(problem::EstimationProblem, solver::IDWSolverHIP) =
  neighbor_estimate(problem, solver, "_distance", u -> NoUnits, (p, X, z, n, d, X0, m, k, radius, ir, μ, aux, status) -> begin
    @assert p.exponent > 0 "exponent must be positive"                   # idw.jl:96
    met, mpar = searchmetric(p)
    ccall((:gss_idw_predict, libgss), Int32,
          (Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Float64}, Int64, Int32, Int32, Float64, Ptr{Float64},
           Int32, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Int32, Ptr{Cvoid}),
          X, z, n, Int32(d), X0, m, k, Int32(p.minneighbors), radius, ir, met, mpar, Float64(p.exponent), μ, aux,
          status, GSS_MEM_HOST, C_NULL)
  end, (p, X, L, n, d, D, X0, m, k, radius, ir, M, aux, status) -> begin
    @assert p.exponent > 0 "exponent must be positive"
    met, mpar = searchmetric(p)
    ccall((:gss_idw_predict_cols, libgss), Int32,
          (Ptr{Float64}, Ptr{Float64}, Int64, Int32, Int32, Ptr{Float64}, Int64, Int32, Int32, Float64, Ptr{Float64},
           Int32, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Int32, Ptr{Cvoid}),
          X, L, n, Int32(d), D, X0, m, k, Int32(p.minneighbors), radius, ir, met, mpar, Float64(p.exponent), M, aux,
          status, GSS_MEM_HOST, C_NULL)
  end)

# an arbitrary `weightfun` closure (lwr.jl:58) cannot cross the C-ABI: the device searches, the weights are evaluated
# here, the device solves the normal equations (gss_lwr_predict_weights)
function lwr_with_closure(p, X, z, n, d, X0, m, k, radius, ir, μ, aux, status)
  met, mpar = searchmetric(p)
  idx = Matrix{Int32}(undef, k, m); cnt = Vector{Int32}(undef, m)          # k x m == m x k row-major
  GC.@preserve X X0 ir idx cnt check(ccall((:gss_knn_search, libgss), Int32,
    (Ptr{Float64}, Int64, Int32, Ptr{Float64}, Int64, Int32, Float64, Ptr{Float64}, Int32, Float64, Ptr{Int32},
     Ptr{Int32}, Int32, Ptr{Cvoid}), X, n, Int32(d), X0, m, k, radius, ir, met, mpar, idx, cnt, GSS_MEM_HOST, C_NULL))
  dist = isnothing(p.neighborhood) ? p.distance : metric(p.neighborhood)   # what the searcher ranks by (ui.jl:25-31)
  W = zeros(Float64, k, m)
  for j in 1:m
    c = Int(cnt[j])
    c == 0 && continue
    ds = [evaluate(dist, view(X, :, Int(idx[i, j]) + 1), view(X0, :, j)) for i in 1:c]
    δs = ds ./ maximum(ds)                                                  # lwr.jl:132
    W[1:c, j] .= p.weightfun.(δs)                                           # lwr.jl:136
  end
  GC.@preserve X z X0 idx cnt W μ aux status ccall((:gss_lwr_predict_weights, libgss), Int32,
    (Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Float64}, Int64, Int32, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float64},
     Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Int32, Ptr{Cvoid}),
    X, z, n, Int32(d), X0, m, k, Int32(p.minneighbors), idx, cnt, W, μ, aux, status, GSS_MEM_HOST, C_NULL)
end

solve(problem::EstimationProblem, solver::LWRSolverHIP) =
  neighbor_estimate(problem, solver, "_variance", u -> u^2, (p, X, z, n, d, X0, m, k, radius, ir, μ, aux, status) -> begin   # lwr.jl:153
    p.weightfun isa Union{ExpWeight,TricubeWeight} ||
      return lwr_with_closure(p, X, z, n, d, X0, m, k, radius, ir, μ, aux, status)
    wk, wa, wp = weightspec(p.weightfun)
    met, mpar = searchmetric(p)
    ccall((:gss_lwr_predict, libgss), Int32,
          (Ptr{Float64}, Ptr{Float64}, Int64, Int32, Ptr{Float64}, Int64, Int32, Int32, Float64, Ptr{Float64},
           Int32, Float64, Int32, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Int32, Ptr{Cvoid}),
          X, z, n, Int32(d), X0, m, k, Int32(p.minneighbors), radius, ir, met, mpar, wk, wa, wp, μ, aux, status,
          GSS_MEM_HOST, C_NULL)
  end, (p, X, L, n, d, D, X0, m, k, radius, ir, M, aux, status) -> begin
    p.weightfun isa Union{ExpWeight,TricubeWeight} ||
      throw(ArgumentError("compositional data with a `weightfun` closure: use ExpWeight / TricubeWeight"))
    wk, wa, wp = weightspec(p.weightfun)
    met, mpar = searchmetric(p)
    ccall((:gss_lwr_predict_cols, libgss), Int32,
          (Ptr{Float64}, Ptr{Float64}, Int64, Int32, Int32, Ptr{Float64}, Int64, Int32, Int32, Float64, Ptr{Float64},
           Int32, Float64, Int32, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Int32, Ptr{Cvoid}),
          X, L, n, Int32(d), D, X0, m, k, Int32(p.minneighbors), radius, ir, met, mpar, wk, wa, wp, M, aux, status,
          GSS_MEM_HOST, C_NULL)
  end)

# ---- simulation solvers: shared pieces ------------------------------------------------------------------------
# Ensemble assembled as GeoStatsBase's loop does it (Dict(var => [Vector...]), SURVEY.md A.6; cookie.jl:82)
function ensemble(problem, reals::Dict)
  Ensemble(domain(problem), reals)
end

# (radius, inv_radii) of the search ball; a rotated ball (searchmetric: GSS_METRIC_ROTATED_BALL) hands 12 doubles:
# three inverse radii, then the row-major rotation
function ballspec(neighborhood)
  radius, ir = -1.0, C_NULL
  if !isnothing(neighborhood)
    rs = ustrip.(radii(neighborhood))
    length(rs) == 1 ? (radius = Float64(rs[1])) : (radius = 1.0; ir = Float64[1 / r for r in rs])
    rot = ballrotation(neighborhood)
    if !isnothing(rot)
      ir = vcat(Float64[i <= length(rs) ? 1 / rs[i] : 1.0 for i in 1:3], collect(rot))
    end
  end
  radius, ir
end

# nearest domain element of every point of X (d x n), 1-based: `search(point, KNearestSearch(pdomain, 1))`, fft.jl:129-132
function nearest_elements(C::Matrix{Float64}, X::Matrix{Float64})
  d, N = size(C)
  n = size(X, 2)
  idx = Vector{Int32}(undef, n); cnt = Vector{Int32}(undef, n)
  GC.@preserve C X idx cnt check(ccall((:gss_knn_search, libgss), Int32,
    (Ptr{Float64}, Int64, Int32, Ptr{Float64}, Int64, Int32, Float64, Ptr{Float64}, Int32, Float64, Ptr{Int32},
     Ptr{Int32}, Int32, Ptr{Cvoid}), C, N, Int32(d), X, n, Int32(1), -1.0, C_NULL, Int32(0), 0.0, idx, cnt,
    GSS_MEM_HOST, C_NULL))
  Int.(idx) .+ 1
end

# The same on a whole CartesianGrid, by arithmetic (mirrors gss/solvers.py `_nearest_cells`): the cell that contains
# the point or a neighbour along an axis, under the search's own rule -- squared distance accumulated in dimension
# order, ties to the lower index -- so that no search index over millions of cells is built (33 ms at 128^3).
# C holds the centroids of the grid (d x N, first axis fastest), used for the candidates' coordinates.
function nearest_cells(C::Matrix{Float64}, dims::Vector{Int64}, origin::Vector{Float64}, sp::Vector{Float64},
                       X::Matrix{Float64})
  d, n = size(X)
  out = Vector{Int}(undef, n)
  strides = cumprod(vcat(1, dims[1:end-1]))
  for i in 1:n
    base = [(t = (X[a, i] - origin[a]) / sp[a]; isfinite(t) ? clamp(floor(Int, t), 0, dims[a] - 1) : 0) for a in 1:d]
    bestd, besti = Inf, typemax(Int)
    for offs in Iterators.product(ntuple(_ -> -1:1, d)...)
      lin = 0
      for a in 1:d
        lin += clamp(base[a] + offs[a], 0, dims[a] - 1) * strides[a]
      end
      acc = 0.0
      for a in 1:d
        t = C[a, lin + 1] - X[a, i]
        acc += t * t
      end
      if acc < bestd || (acc == bestd && lin < besti)
        bestd, besti = acc, lin
      end
    end
    out[i] = besti + 1
  end
  out
end

# ---- FFTGS ----------------------------------------------------------------------------------
@simsolver FFTGSHIP begin
  @param variogram = GaussianVariogram()
  @param mean = 0.0
  @param minneighbors = 1
  @param maxneighbors = nothing
  @param neighborhood = nothing
  @param distance = Euclidean()
  @global threads = Sys.CPU_THREADS    # accepted like fft.jl:58; there is no FFTW thread pool to configure
  @global rng = Random.GLOBAL_RNG      # fft.jl:59: the Philox seed of a solve is `rand(rng, UInt64)`
end

preprocess(problem::SimulationProblem, solver::FFTGSHIP) = fftgs_preprocess(problem, solver)

# `compute=false`: the spectrum arrives from another process (import_token!); `seed`: the run's Philox seed when the
# caller has drawn it already (every worker of a distributed solve must use the same one)
function fftgs_preprocess(problem::SimulationProblem, solver::FFTGSHIP; compute=true, seed=nothing)
  pdata = data(problem)
  pdomain = domain(problem)
  pgrid = parent(pdomain)
  dims = Int64[size(pgrid)...]
  sp = Float64[ustrip.(spacing(pgrid))...]
  preproc = Dict{Any,Any}()
  for covars in covariables(problem, solver), var in covars.names
    p = covars.params[Set([var])]
    γ, μ = p.variogram, p.mean
    vg = Ref(cvariogram(γ, length(dims)))                                # throws ArgumentError if not stationary, fft.jl:91-93
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:gss_fftgs_create, libgss), Int32,
                (Ptr{Ptr{Cvoid}}, Ptr{GssVariogram}, Int32, Ptr{Int64}, Ptr{Float64}, Float64, Int32, Ptr{Cvoid}),
                h, vg, Int32(length(dims)), dims, sp, Float64(μ), compute ? Int32(0) : GSS_FFTGS_NO_SPECTRUM,
                C_NULL))                                                   # fft.jl:96-103
    handle = Handle(h[], :fftgs)
    # conditional simulation, fft.jl:105-135: krige the data, locate the data cells
    z̄, krig, dinds = nothing, nothing, nothing
    if !isnothing(pdata)
      dtable = values(pdata)
      ddomain = domain(pdata)
      if var ∈ Tables.schema(dtable).names
        kdat = georef(dtable, centroid.(ddomain))
        kdom = PointSet(centroid.(pdomain))
        prob = EstimationProblem(kdat, kdom, var)
        krig = KrigingSolverHIP(var => (variogram=γ, mean=μ, minneighbors=p.minneighbors, maxneighbors=p.maxneighbors,
                                        neighborhood=p.neighborhood, distance=p.distance))
        z̄ = getproperty(solve(prob, krig), var)                          # fft.jl:125-126
        C = coordmatrix(pdomain)
        found = pdomain isa CartesianGrid ?
                nearest_cells(C, dims, Float64[ustrip.(coordinates(minimum(pgrid)))...], sp, coordmatrix(ddomain)) :
                nearest_elements(C, coordmatrix(ddomain))               # fft.jl:129-131
        dinds = unique(found)                                            # fft.jl:132
      end
    end
    preproc[var] = (γ=γ, μ=μ, handle=handle, z̄=z̄, krig=krig, dinds=dinds, maxneighbors=p.maxneighbors)
  end
  preproc[:_run] = RunState(problem, solver; seed)
  preproc
end

# realisations first .. first+count-1 of `var` on the problem domain, npts x count (fft.jl:163-173 for each)
function fftgs_block(problem, preproc, var, first::Int, count::Int)
  pdomain = domain(problem)
  npts = nelements(pdomain)
  ii = Int64.(collect(parentindices(pdomain)) .- 1)                      # 0-based on the C side, fft.jl:152,173
  out = Matrix{Float64}(undef, npts, count)
  count == 0 && return out
  par = preproc[var]
  GC.@preserve out ii check(ccall((:gss_fftgs_realize, libgss), Int32,
    (Ptr{Cvoid}, UInt64, Int64, Int64, Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Float64}, Int32, Ptr{Cvoid}),
    par.handle, varseed(preproc[:_run], var), Int64(first), Int64(count), C_NULL, ii, Int64(npts), out, GSS_MEM_HOST,
    C_NULL))
  isnothing(par.krig) && return out
  # conditioning, fft.jl:176-192: krige the unconditional values at the data cells, add the residual field
  if isnothing(par.maxneighbors)
    # global neighbourhood: the kriging system of fft.jl:187 has the same locations (the data cells' centroids) for
    # every realisation -- ONE factorisation, the realisations' values at the data cells as a batch of right-hand
    # sides (means only: gss_krig_predict_global_batch), instead of a solve(EstimationProblem...) per realisation
    X0 = coordmatrix(pdomain)
    d, m = size(X0)
    Xd = X0[:, par.dinds]
    nd = length(par.dinds)
    Zb = out[par.dinds, :]                                              # nd x count == count x nd row-major
    Z̄ᵤ = Matrix{Float64}(undef, m, count)
    vg = Ref(cvariogram(par.γ, d))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    z0 = Zb[:, 1]
    GC.@preserve X0 Xd Zb Z̄ᵤ z0 begin
      check(ccall((:gss_krig_create, libgss), Int32,
                  (Ptr{Ptr{Cvoid}}, Ptr{GssVariogram}, Int32, Float64, Int32, Int32, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Int64, Int32, Ptr{Cvoid}),
                  h, vg, Int32(0), Float64(par.μ), Int32(0), Int32(0), Xd, z0, C_NULL, nd, Int32(0), C_NULL))
      try
        check(ccall((:gss_krig_predict_global_batch, libgss), Int32,
                    (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int32, Ptr{Cvoid}),
                    h[], X0, m, Zb, count, Z̄ᵤ, GSS_MEM_HOST, C_NULL))
      finally
        ccall((:gss_krig_destroy, libgss), Int32, (Ptr{Cvoid},), h[])
      end
    end
    out .= par.z̄ .+ (out .- Z̄ᵤ)                                         # fft.jl:191
    return out
  end
  kdom = PointSet(centroid.(pdomain))
  ddomain = view(pdomain, par.dinds)
  for r in 1:count
    zᵤ = view(out, :, r)
    kdat = georef((; var => zᵤ[par.dinds]), centroid.(ddomain))
    z̄ᵤ = getproperty(solve(EstimationProblem(kdat, kdom, var), par.krig), var)
    zᵤ .= par.z̄ .+ (zᵤ .- z̄ᵤ)                                            # fft.jl:191
  end
  out
end

function solvesingle(problem::SimulationProblem, covars::NamedTuple, solver::FFTGSHIP, preproc)
  r = nextreal!(preproc[:_run], covars.names)
  Dict(var => fftgs_block(problem, preproc, var, r, 1)[:, 1] for var in covars.names)
end

function solve(problem::SimulationProblem, solver::FFTGSHIP; procs=[myid()])
  procs == [myid()] || return solve_on_workers(problem, solver, collect(procs))
  preproc = preprocess(problem, solver)
  reals = Dict{Symbol,Vector{Vector{Float64}}}()
  for covars in covariables(problem, solver), var in covars.names
    Z = fftgs_block(problem, preproc, var, 0, nreals(problem))           # one device call for all realisations
    reals[var] = [Z[:, r] for r in 1:nreals(problem)]
    destroy!(preproc[var].handle)
  end
  ensemble(problem, reals)
end

# ---- LUGS -------------------------------------------------------------------------------------
@simsolver LUGSHIP begin
  @param variogram = GaussianVariogram()
  @param mean = nothing
  @param factorization = cholesky
  @jparam correlation = 0.0
  @global init = NearestInit()
  @global rng = Random.GLOBAL_RNG      # lu.jl:73
end

preprocess(problem::SimulationProblem, solver::LUGSHIP) = lugs_preprocess(problem, solver)

function lugs_preprocess(problem::SimulationProblem, solver::LUGSHIP; compute=true, seed=nothing)
  pdomain = domain(problem)
  buff, mask = initbuff(pdomain, variables(problem), solver.init, data=data(problem))   # lu.jl:86
  C = coordmatrix(pdomain)
  d, N = size(C)
  preproc = Dict{Any,Any}()
  for covars in covariables(problem, solver)
    conames = covars.names
    @assert length(conames) ∈ (1, 2) "invalid number of covariables"                    # lu.jl:96
    coparams = Dict{Any,Any}()
    for var in conames
      p = covars.params[Set([var])]
      dlocs = Int64.(findall(mask[var]) .- 1)                                           # lu.jl:113
      z₁ = Float64.(buff[var][findall(mask[var])])
      !isnothing(p.mean) && !isempty(dlocs) && @warn "mean can only be specified in unconditional simulation"
      μ = isnothing(p.mean) ? 0.0 : Float64(p.mean)
      flags = (p.factorization === cholesky ? Int32(0) : GSS_LUGS_FACT_LU) |           # lu.jl:70,107
              (compute ? Int32(0) : GSS_LUGS_NO_FACTOR)
      vg = Ref(cvariogram(p.variogram, d))
      h = Ref{Ptr{Cvoid}}(C_NULL)
      GC.@preserve C dlocs z₁ check(ccall((:gss_lugs_create, libgss), Int32,
        (Ptr{Ptr{Cvoid}}, Ptr{GssVariogram}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Float64}, Int64, Float64, Int32,
         Ptr{Cvoid}), h, vg, C, N, dlocs, z₁, length(dlocs), μ, flags, C_NULL))
      coparams[Set([var])] = (handle=Handle(h[], :lugs), N=N, ns=N - length(dlocs))
    end
    length(conames) == 2 && (coparams[conames] = covars.params[conames].correlation)    # lu.jl:154-163
    push!(preproc, conames => coparams)
  end
  preproc[:_run] = RunState(problem, solver; seed)
  preproc
end

# lusim (lu.jl:198-224) for realisations first .. first+count-1: (N x count fields, ns x count normals used)
function lusim_hip(par, seed, first::Int, count::Int, ρ=nothing, W₁=nothing)
  Y = Matrix{Float64}(undef, par.N, count)
  W₂ = Matrix{Float64}(undef, par.ns, count)
  count == 0 && return Y, W₂
  GC.@preserve Y W₂ W₁ check(ccall((:gss_lugs_realize, libgss), Int32,
    (Ptr{Cvoid}, UInt64, Int64, Int64, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int32,
     Ptr{Cvoid}), par.handle, seed, Int64(first), Int64(count), C_NULL, isnothing(ρ) ? 0.0 : Float64(ρ),
    isnothing(W₁) ? C_NULL : pointer(W₁), Y, W₂, GSS_MEM_HOST, C_NULL))
  Y, W₂
end

function lugs_block(preproc, conames, first::Int, count::Int)                            # lu.jl:171-196
  run = preproc[:_run]
  coparams = preproc[conames]
  vars = collect(conames)
  v₁ = Base.first(vars)
  Y₁, W₁ = lusim_hip(coparams[Set([v₁])], varseed(run, v₁), first, count)
  result = Dict{Symbol,Matrix{Float64}}(v₁ => Y₁)
  if length(conames) == 2
    v₂ = last(vars)
    Y₂, _ = lusim_hip(coparams[Set([v₂])], varseed(run, v₂), first, count, coparams[conames], W₁)
    result[v₂] = Y₂
  end
  result
end

function solvesingle(::SimulationProblem, covars::NamedTuple, solver::LUGSHIP, preproc)
  r = nextreal!(preproc[:_run], covars.names)
  Dict(var => Y[:, 1] for (var, Y) in lugs_block(preproc, covars.names, r, 1))
end

function solve(problem::SimulationProblem, solver::LUGSHIP; procs=[myid()])
  procs == [myid()] || return solve_on_workers(problem, solver, collect(procs))
  preproc = preprocess(problem, solver)
  reals = Dict{Symbol,Vector{Vector{Float64}}}()
  for covars in covariables(problem, solver)
    for (var, Y) in lugs_block(preproc, covars.names, 0, nreals(problem))   # one GEMM L22 * W for all realisations
      reals[var] = [Y[:, r] for r in 1:nreals(problem)]
      destroy!(preproc[covars.names][Set([var])].handle)
    end
  end
  ensemble(problem, reals)
end

# ---- device-resident arrays (GSS_MEM_DEVICE) -------------------------------------------------------------------------
# The solver methods above take and return host arrays, like the reference.  A caller that keeps its arrays in HBM
# (AMDGPU.jl: `pointer(A)` of a `ROCArray{Float64}` on the device this process is bound to) uses these entry points:
# nothing crosses PCIe and the calls are asynchronous on `stream` (a hipStream_t as Ptr{Cvoid}; C_NULL = default stream).
struct KrigingFit
  handle::Handle
  n::Int
  d::Int
end

"""
    krig_fit(γ, X, z; mean=nothing, degree=nothing) -> KrigingFit

Factorise the kriging system of the data `X` (d x n, host) / `z` once on the device (krig.jl:176); `mean` selects simple
kriging, `degree` universal kriging, neither ordinary kriging (ui.jl:40-50).
"""
function krig_fit(γ, X::Matrix{Float64}, z::Vector{Float64}; mean=nothing, degree=nothing)
  d, n = size(X)
  variant, deg, skmean = Int32(1), Int32(0), 0.0
  if !isnothing(degree)
    variant, deg = Int32(2), Int32(degree)
  elseif !isnothing(mean)
    variant, skmean = Int32(0), Float64(mean)
  end
  extent = sqrt(sum(abs2, maximum(X, dims=2) .- minimum(X, dims=2)))
  vg = Ref(cvariogram(γ, d; extent))
  h = Ref{Ptr{Cvoid}}(C_NULL)
  GC.@preserve X z check(ccall((:gss_krig_create, libgss), Int32,
    (Ptr{Ptr{Cvoid}}, Ptr{GssVariogram}, Int32, Float64, Int32, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64,
     Int32, Ptr{Cvoid}), h, vg, variant, skmean, deg, Int32(0), X, z, C_NULL, n, Int32(0), C_NULL))
  KrigingFit(Handle(h[], :krig), n, d)
end

"""
    krig_predict_device!(μ, σ², status, fit, X0, m; stream=C_NULL)

Global-neighbourhood estimates (krig.jl:180-183) at the `m` points whose coordinates (d x m, column-major) sit in HBM at
`X0`; means, variances and status bytes are written to HBM at `μ`, `σ²`, `status`.
"""
function krig_predict_device!(μ::Ptr{Float64}, σ²::Ptr{Float64}, status::Ptr{UInt8}, fit::KrigingFit, X0::Ptr{Float64},
                              m::Integer; stream::Ptr{Cvoid}=C_NULL)
  check(ccall((:gss_krig_predict_global, libgss), Int32,
              (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Int32, Ptr{Cvoid}),
              fit.handle, X0, C_NULL, Int64(m), μ, σ², status, GSS_MEM_DEVICE, stream))
end

# ---- cross-validation (gss.h: gss_krig_cv_global, gss_krig_cv_global_folds, gss_krig_cv_knn, gss_cv_summary) ----
struct CVSummary
  n_ok::Float64
  n_missing::Float64
  n_singular::Float64
  me::Float64
  mae::Float64
  mse::Float64
  mse_std_n::Float64
  mean_std::Float64
  msq_std::Float64
  cverror::Float64
end

"""
    krig_cv_global(fit) -> (pred, σ², status)

Leave-one-out prediction of every sample of `fit = krig_fit(...)` under the global neighbourhood, read off the factor.
"""
function krig_cv_global(fit::KrigingFit)
  pred = Vector{Float64}(undef, fit.n); σ² = similar(pred); status = Vector{UInt8}(undef, fit.n)
  GC.@preserve pred σ² status check(ccall((:gss_krig_cv_global, libgss), Int32,
    (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Int32, Ptr{Cvoid}), fit.handle, pred, σ², status, GSS_MEM_HOST,
    C_NULL))
  pred, σ², status
end

"""
    cv_summary(z, pred, σ², status; folds=nothing, nfolds=0) -> (CVSummary, per-fold mean squared errors or nothing)

`folds`: 0-based fold ids (Int32) of the samples, `nothing` for leave-one-out.
"""
function cv_summary(z::Vector{Float64}, pred::Vector{Float64}, σ²::Vector{Float64}, status::Vector{UInt8};
                    folds::Union{Nothing,Vector{Int32}}=nothing, nfolds::Integer=0)
  out = Ref(CVSummary(0, 0, 0, 0, 0, 0, 0, 0, 0, 0))
  nf = isnothing(folds) ? 0 : Int(nfolds)
  fmse = nf > 0 ? Vector{Float64}(undef, nf) : nothing
  GC.@preserve z pred σ² status folds fmse check(ccall((:gss_cv_summary, libgss), Int32,
    (Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Int32}, Int64, Int32, Ptr{Cvoid}, Ptr{Float64}, Int32,
     Ptr{Cvoid}), z, pred, σ², status, isnothing(folds) ? C_NULL : folds, Int64(length(z)), Int32(nf), out,
    isnothing(fmse) ? C_NULL : fmse, GSS_MEM_HOST, C_NULL))
  out[], fmse
end

"""
    cverror(solver::KrigingSolverHIP, problem; folds=nothing, excluderadius=nothing) -> Dict(var => error)

Cross-validation error of every variable of `problem` on its own samples (the domain is not used): the mean over the
folds of the folds' mean squared errors.  `folds`: 0-based fold id per non-missing sample (`nothing`: leave-one-out);
`excluderadius`: leave-ball-out.  `maxneighbors = nothing` is the global neighbourhood: leave-one-out and `folds` are both
read off the factor of the one fitted system (no refit per fold); `excluderadius` there throws, a ball is no partition
of the samples.
"""
function cverror(solver::KrigingSolverHIP, problem::EstimationProblem; folds=nothing, excluderadius=nothing)
  pdata = data(problem)
  dtable = values(pdata)
  ddomain = domain(pdata)
  errs = Dict{Symbol,Float64}()
  for covars in covariables(problem, solver), var in covars.names
    p = covars.params[Set([var])]
    zcol = Tables.getcolumn(Tables.columns(dtable), var)
    inds = findall(!ismissing, zcol)
    z, u = stripunits(zcol)
    X = coordmatrix(view(ddomain, inds))
    d, n = size(X)
    variant, degree, ndrift, Fd, skmean = Int32(1), Int32(0), Int32(0), C_NULL, 0.0
    if !isnothing(p.drifts)
      variant, ndrift = Int32(3), Int32(length(p.drifts))
      Fd = Float64[f(Point(X[:, i]...)) for f in p.drifts, i in 1:n]
    elseif !isnothing(p.degree)
      variant, degree = Int32(2), Int32(p.degree)
    elseif !isnothing(p.mean)
      variant, skmean = Int32(0), (p.mean isa Quantity ? Float64(ustrip(u, p.mean)) : Float64(p.mean))
    end
    exact = isnothing(p.maxneighbors)
    exact && !isnothing(excluderadius) &&
      throw(ArgumentError("the global neighbourhood (maxneighbors = nothing) offers leave-one-out and folds only"))
    p.support === :point || throw(ArgumentError("cross-validation is at point support"))
    extent = sqrt(sum(abs2, maximum(X, dims=2) .- minimum(X, dims=2)))
    vg = Ref(cvariogram(p.variogram, d; extent))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    pred = Vector{Float64}(undef, n); σ² = similar(pred); status = Vector{UInt8}(undef, n)
    fold = isnothing(folds) ? nothing : Vector{Int32}(folds)
    GC.@preserve X z Fd pred σ² status fold begin
      check(ccall((:gss_krig_create, libgss), Int32,
                  (Ptr{Ptr{Cvoid}}, Ptr{GssVariogram}, Int32, Float64, Int32, Int32, Ptr{Float64}, Ptr{Float64},
                   Ptr{Float64}, Int64, Int32, Ptr{Cvoid}),
                  h, vg, variant, skmean, degree, ndrift, X, z, Fd, n, exact ? Int32(0) : GSS_KRIG_NO_FACTOR, C_NULL))
      try
        if exact && isnothing(fold)
          check(ccall((:gss_krig_cv_global, libgss), Int32,
                      (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Int32, Ptr{Cvoid}),
                      h[], pred, σ², status, GSS_MEM_HOST, C_NULL))
        elseif exact
          check(ccall((:gss_krig_cv_global_folds, libgss), Int32,
                      (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Int32, Ptr{Cvoid}),
                      h[], fold, pred, σ², status, GSS_MEM_HOST, C_NULL))
        else
          radius, ir = ballspec(p.neighborhood)
          met, mpar = searchmetric(p)
          k = clamp(p.maxneighbors, 1, n - 1)
          check(ccall((:gss_krig_cv_knn, libgss), Int32,
                      (Ptr{Cvoid}, Ptr{Int32}, Float64, Int32, Int32, Float64, Ptr{Float64}, Int32, Float64, Ptr{Float64},
                       Ptr{Float64}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Cvoid}),
                      h[], isnothing(fold) ? C_NULL : fold, isnothing(excluderadius) ? -1.0 : Float64(excluderadius),
                      Int32(k), Int32(p.minneighbors), radius, ir, met, mpar, pred, σ², status, C_NULL, C_NULL,
                      GSS_MEM_HOST, C_NULL))
        end
      finally
        ccall((:gss_krig_destroy, libgss), Int32, (Ptr{Cvoid},), h[])
      end
    end
    nf = isnothing(fold) ? 0 : Int(maximum(fold)) + 1
    s, _ = cv_summary(Vector{Float64}(z), pred, σ², status; folds=fold, nfolds=nf)
    errs[var] = s.cverror
  end
  errs
end

"""
    fftgs_realize_device!(dst, preproc, var, first, count; stream=C_NULL)

Unconditional realisations `first .. first+count-1` of `var` on the whole grid of `preproc = preprocess(problem,
solver::FFTGSHIP)`, written to HBM at `dst` (count x N doubles, realisation-major) -- the 500+ realisations/s path;
`solve` / `solvesingle` deliver host vectors like the reference and are bounded by PCIe (~50 realisations/s at 512^3).
"""
function fftgs_realize_device!(dst::Ptr{Float64}, preproc, var::Symbol, first::Integer, count::Integer;
                               stream::Ptr{Cvoid}=C_NULL)
  check(ccall((:gss_fftgs_realize, libgss), Int32,
              (Ptr{Cvoid}, UInt64, Int64, Int64, Ptr{Float64}, Ptr{Int64}, Int64, Ptr{Float64}, Int32, Ptr{Cvoid}),
              preproc[var].handle, varseed(preproc[:_run], var), Int64(first), Int64(count), C_NULL, C_NULL, Int64(0),
              dst, GSS_MEM_DEVICE, stream))
end

# ---- variography: replaces Variography's EmpiricalVariogram / DirectionalVariogram / fit (include/gss.h) ----------
const GAMMA_CONSTRUCTORS = (GaussianVariogram, ExponentialVariogram, SphericalVariogram, MaternVariogram, CubicVariogram,
                            PentasphericalVariogram, SineHoleVariogram)          # index - 1 = GSS_VG_*

"""
    empirical_variogram(data, vars; nlags=20, maxlag=nothing, estimator=:matheron, direction=nothing, dtol=Inf, atol=π/8)

Empirical variogram(s) of the variable(s) `vars` (a Symbol or a collection of up to 8 Symbols measured on the same samples:
one pass over the pairs serves them all) on the device.  `maxlag` defaults to a tenth of the diagonal of the samples'
bounding box ([RECALL] Variography's default); `direction` (any non-zero vector) keeps the pairs inside a band of
half-width `dtol` and a cone of half-angle `atol` about it, either sense.  Rows with a missing value in any of `vars`
are dropped.  Returns `(abscissa, ordinate, counts, nduplicates)`; `ordinate` is a Dict var => Vector for several
variables.  Bins without pairs hold NaN.
"""
function empirical_variogram(data, vars; nlags::Integer=20, maxlag=nothing, estimator::Symbol=:matheron,
                             direction=nothing, dtol::Real=Inf, atol::Real=π / 8)
  names = vars isa Symbol ? [vars] : collect(Symbol, vars)
  tab = Tables.columns(values(data))
  cols = [Tables.getcolumn(tab, v) for v in names]
  keep = [i for i in 1:nelements(domain(data)) if all(c -> !ismissing(c[i]) && isfinite(ustrip(c[i])), cols)]
  X = coordmatrix(domain(data))[:, keep]
  d, n = size(X)
  Z = Matrix{Float64}(undef, n, length(names))          # column c at Z + c * n
  for (c, col) in enumerate(cols), (r, i) in enumerate(keep)
    Z[r, c] = Float64(ustrip(col[i]))
  end
  lag = isnothing(maxlag) ? 0.1 * sqrt(sum(abs2, maximum(X, dims=2) .- minimum(X, dims=2))) : Float64(ustrip(maxlag))
  u = isnothing(direction) ? nothing : collect(Float64, direction) ./ sqrt(sum(abs2, direction))
  cosatol = isnothing(direction) || atol >= π / 2 ? 0.0 : cos(Float64(atol))
  est = estimator == :cressie ? Int32(1) : Int32(0)
  count = Vector{Int64}(undef, nlags)
  lagsum = Vector{Float64}(undef, nlags)
  zsum = Matrix{Float64}(undef, nlags, length(names))
  ndup = Ref{Int64}(0)
  GC.@preserve X Z u check(ccall((:gss_variogram_empirical, libgss), Int32,
    (Ptr{Float64}, Int64, Int32, Ptr{Float64}, Int32, Int32, Float64, Ptr{Float64}, Float64, Float64, Int32, Ptr{Int64},
     Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Int32, Ptr{Cvoid}),
    X, Int64(n), Int32(d), Z, Int32(length(names)), Int32(nlags), lag, isnothing(u) ? C_NULL : pointer(u), Float64(dtol),
    cosatol, est, count, lagsum, zsum, ndup, GSS_MEM_HOST, C_NULL))
  abscissa = [c > 0 ? s / c : NaN for (s, c) in zip(lagsum, count)]
  gamma(col) = [c == 0 ? NaN : est == 0 ? s / 2c : (s / c)^4 / (2 * (0.457 + 0.494 / c)) for (s, c) in zip(col, count)]
  ordinate = vars isa Symbol ? gamma(zsum[:, 1]) : Dict(v => gamma(zsum[:, c]) for (c, v) in enumerate(names))
  (abscissa=abscissa, ordinate=ordinate, counts=count, nduplicates=ndup[])
end

"""
    fit_variogram(kinds, abscissa, ordinate, counts; weighting=:count, order=1.0, maxnuggetfrac=1.0)

Weighted least-squares fit (gss_variogram_fit, host code of the library) of the best of `kinds` -- variogram types such
as `GaussianVariogram`, or one of them -- to an empirical variogram; returns the Variography model.  The library fits
the Gaussian kind as the bare formula: the nugget handed to `GaussianVariogram` is the fitted one minus the constant
the loaded Variography adds on evaluation (GAUSSIAN_NUGGET_EPS), not below zero.
"""
function fit_variogram(kinds, abscissa::Vector{Float64}, ordinate::Vector{Float64}, counts::Vector{Int64};
                       weighting::Symbol=:count, order::Real=1.0, maxnuggetfrac::Real=1.0)
  ks = kinds isa Type ? [kinds] : collect(kinds)
  codes = Int32[something(findfirst(==(k), GAMMA_CONSTRUCTORS), 8) - 1 for k in ks]      # anything else: GSS_VG_POWER
  w = weighting == :count ? Int32(0) : weighting == :uniform ? Int32(2) : Int32(1)
  best = Ref(cvariogram(GaussianVariogram(), 1))
  objective = Vector{Float64}(undef, length(codes))
  check(ccall((:gss_variogram_fit, libgss), Int32,
    (Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Int32, Ptr{Int32}, Int32, Float64, Int32, Float64, Ptr{GssVariogram},
     Ptr{Float64}), abscissa, ordinate, counts, Int32(length(counts)), codes, Int32(length(codes)), Float64(order), w,
    Float64(maxnuggetfrac), best, objective))
  b = best[]
  T = GAMMA_CONSTRUCTORS[b.kind+1]
  nug = T === GaussianVariogram ? max(b.nugget - GAUSSIAN_NUGGET_EPS[], 0.0) : b.nugget
  T === MaternVariogram ? T(sill=b.sill, nugget=nug, range=b.range, order=b.nu) : T(sill=b.sill, nugget=nug, range=b.range)
end

"""
    empirical_varioplane(data, vars; nangs=18, nlags=20, maxlag=nothing, offset=0.0, normal=nothing, ptol=Inf,
                         estimator=:matheron)

Empirical variogram of every one of `nangs` equal direction sectors of the half-circle in ONE pass over the pairs
(gss_variogram_plane): sector s holds the directions [offset + (s-1)π/nangs, offset + sπ/nangs) modulo π.  2-D data: the
plane of the samples (`normal` is refused); 3-D data: `normal` is required, the in-plane axes are built as the twin's
`plane_basis` builds them (e1 = the coordinate axis with the smallest |component| of the unit normal, made orthogonal to
it; e2 = n × e1) and pairs farther than `ptol` from the plane are left out.  Up to 4 variables measured on the same
samples with `nangs * nlags * (2 + length(vars)) <= 8192`.  Returns `(angles, midangles, abscissa, ordinate, counts,
nduplicates)` with `nlags × nangs` matrices (sector s in column s); `ordinate` is a Dict for several variables.
"""
function empirical_varioplane(data, vars; nangs::Integer=18, nlags::Integer=20, maxlag=nothing, offset::Real=0.0,
                              normal=nothing, ptol::Real=Inf, estimator::Symbol=:matheron)
  names = vars isa Symbol ? [vars] : collect(Symbol, vars)
  tab = Tables.columns(values(data))
  cols = [Tables.getcolumn(tab, v) for v in names]
  keep = [i for i in 1:nelements(domain(data)) if all(c -> !ismissing(c[i]) && isfinite(ustrip(c[i])), cols)]
  X = coordmatrix(domain(data))[:, keep]
  d, n = size(X)
  d == 2 && !isnothing(normal) && throw(ArgumentError("normal describes a plane in 3-D; 2-D samples lie in their own plane"))
  d == 3 && isnothing(normal) && throw(ArgumentError("3-D samples need the normal of the plane"))
  basis = nothing
  if d == 3
    nrm = collect(Float64, normal) ./ sqrt(sum(abs2, normal))
    a = zeros(3); a[argmin(abs.(nrm))] = 1.0
    e1 = a .- sum(a .* nrm) .* nrm; e1 ./= sqrt(sum(abs2, e1))
    e2 = [nrm[2] * e1[3] - nrm[3] * e1[2], nrm[3] * e1[1] - nrm[1] * e1[3], nrm[1] * e1[2] - nrm[2] * e1[1]]
    e2 ./= sqrt(sum(abs2, e2))
    basis = vcat(e1, e2, nrm)
  end
  Z = Matrix{Float64}(undef, n, length(names))
  for (c, col) in enumerate(cols), (r, i) in enumerate(keep)
    Z[r, c] = Float64(ustrip(col[i]))
  end
  lag = isnothing(maxlag) ? 0.1 * sqrt(sum(abs2, maximum(X, dims=2) .- minimum(X, dims=2))) : Float64(ustrip(maxlag))
  angles = [Float64(offset) + (s - 1) * π / nangs for s in 1:nangs]
  dirs = Matrix{Float64}(undef, 2, nangs)               # (cos, sin) of sector s at dirs + 2 (s - 1)
  for s in 1:nangs
    dirs[1, s] = cos(angles[s]); dirs[2, s] = sin(angles[s])
  end
  est = estimator == :cressie ? Int32(1) : Int32(0)
  count = Matrix{Int64}(undef, nlags, nangs)
  lagsum = Matrix{Float64}(undef, nlags, nangs)
  zsum = Array{Float64,3}(undef, nlags, nangs, length(names))
  ndup = Ref{Int64}(0)
  GC.@preserve X Z dirs basis check(ccall((:gss_variogram_plane, libgss), Int32,
    (Ptr{Float64}, Int64, Int32, Ptr{Float64}, Int32, Int32, Float64, Int32, Ptr{Float64}, Ptr{Float64}, Float64, Int32,
     Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Int32, Ptr{Cvoid}),
    X, Int64(n), Int32(d), Z, Int32(length(names)), Int32(nlags), lag, Int32(nangs), dirs,
    isnothing(basis) ? C_NULL : pointer(basis), Float64(ptol), est, count, lagsum, zsum, ndup, GSS_MEM_HOST, C_NULL))
  abscissa = [c > 0 ? s / c : NaN for (s, c) in zip(lagsum, count)]
  gamma(m) = [c == 0 ? NaN : est == 0 ? s / 2c : (s / c)^4 / (2 * (0.457 + 0.494 / c)) for (s, c) in zip(m, count)]
  ordinate = vars isa Symbol ? gamma(zsum[:, :, 1]) : Dict(v => gamma(zsum[:, :, c]) for (c, v) in enumerate(names))
  (angles=angles, midangles=angles .+ π / (2nangs), abscissa=abscissa, ordinate=ordinate, counts=count, nduplicates=ndup[])
end

"""
    fit_anisotropic(kinds, plane; var=nothing, weighting=:count, order=1.0, maxnuggetfrac=1.0)

Fit of 2-D geometric anisotropy (gss_variogram_fit_aniso, host code of the library) to the result of
`empirical_varioplane` (`var` selects the variable when it holds several): returns
`Kind(MetricBall((r1, r2), Angle2d(θ)); sill, nugget)` with r1 >= r2, or the isotropic model when the fitted ratio is 1.
The Gaussian nugget rule is that of `fit_variogram`.
"""
function fit_anisotropic(kinds, plane; var=nothing, weighting::Symbol=:count, order::Real=1.0, maxnuggetfrac::Real=1.0)
  ks = kinds isa Type ? [kinds] : collect(kinds)
  codes = Int32[something(findfirst(==(k), GAMMA_CONSTRUCTORS), 8) - 1 for k in ks]      # anything else: GSS_VG_POWER
  w = weighting == :count ? Int32(0) : weighting == :uniform ? Int32(2) : Int32(1)
  g = plane.ordinate isa Dict ? plane.ordinate[var] : plane.ordinate
  h = vec(collect(Float64, plane.abscissa))
  gam = vec(collect(Float64, g))
  cnt = vec(collect(Int64, plane.counts))
  phi = vec(Float64[plane.midangles[s] for _ in 1:size(plane.counts, 1), s in 1:size(plane.counts, 2)])
  best = Ref(cvariogram(GaussianVariogram(), 1))
  objective = Vector{Float64}(undef, length(codes))
  check(ccall((:gss_variogram_fit_aniso, libgss), Int32,
    (Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Int32, Ptr{Int32}, Int32, Float64, Int32, Float64,
     Ptr{GssVariogram}, Ptr{Float64}), h, phi, gam, cnt, Int32(length(cnt)), codes, Int32(length(codes)), Float64(order),
    w, Float64(maxnuggetfrac), best, objective))
  b = best[]
  T = GAMMA_CONSTRUCTORS[b.kind+1]
  nug = T === GaussianVariogram ? max(b.nugget - GAUSSIAN_NUGGET_EPS[], 0.0) : b.nugget
  if b.aniso == 0
    return T === MaternVariogram ? T(sill=b.sill, nugget=nug, range=b.range, order=b.nu) : T(sill=b.sill, nugget=nug, range=b.range)
  end
  # [RECALL] Meshes exports Rotations' Angle2d (its docs write `Rotate(Angle2d(π/2))`); rotation[1], rotation[4] = cos, sin
  ball = MetricBall((1 / b.inv_radii[1], 1 / b.inv_radii[2]), Angle2d(atan(b.rotation[4], b.rotation[1])))
  T === MaternVariogram ? T(ball; sill=b.sill, nugget=nug, order=b.nu) : T(ball; sill=b.sill, nugget=nug)
end

"""
    empirical_cross_variogram(data, vars; nlags=20, maxlag=nothing, direction=nothing, dtol=Inf, atol=π/8)

Direct and cross variograms (Matheron) of up to 8 variables measured on the same samples in ONE pass over the pairs
(gss_variogram_cross).  Rows with a missing value in any of `vars` are dropped.  Returns `(vars, abscissa, ordinate,
counts, nduplicates)`; `ordinate` is an `nlags × nz(nz+1)/2` matrix whose column `pairindex(nz, a, b)` holds
γ_ab = csum / 2count for the variables a ≤ b (1-based positions in `vars`); the columns (a, a) are the direct variograms.
"""
function empirical_cross_variogram(data, vars; nlags::Integer=20, maxlag=nothing, direction=nothing, dtol::Real=Inf,
                                   atol::Real=π / 8)
  names = collect(Symbol, vars)
  tab = Tables.columns(values(data))
  cols = [Tables.getcolumn(tab, v) for v in names]
  keep = [i for i in 1:nelements(domain(data)) if all(c -> !ismissing(c[i]) && isfinite(ustrip(c[i])), cols)]
  X = coordmatrix(domain(data))[:, keep]
  d, n = size(X)
  nz = length(names)
  Z = Matrix{Float64}(undef, n, nz)          # column c at Z + c * n
  for (c, col) in enumerate(cols), (r, i) in enumerate(keep)
    Z[r, c] = Float64(ustrip(col[i]))
  end
  lag = isnothing(maxlag) ? 0.1 * sqrt(sum(abs2, maximum(X, dims=2) .- minimum(X, dims=2))) : Float64(ustrip(maxlag))
  u = isnothing(direction) ? nothing : collect(Float64, direction) ./ sqrt(sum(abs2, direction))
  cosatol = isnothing(direction) || atol >= π / 2 ? 0.0 : cos(Float64(atol))
  count = Vector{Int64}(undef, nlags)
  lagsum = Vector{Float64}(undef, nlags)
  csum = Matrix{Float64}(undef, nlags, nz * (nz + 1) ÷ 2)
  ndup = Ref{Int64}(0)
  GC.@preserve X Z u check(ccall((:gss_variogram_cross, libgss), Int32,
    (Ptr{Float64}, Int64, Int32, Ptr{Float64}, Int32, Int32, Float64, Ptr{Float64}, Float64, Float64, Ptr{Int64},
     Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Int32, Ptr{Cvoid}),
    X, Int64(n), Int32(d), Z, Int32(nz), Int32(nlags), lag, isnothing(u) ? C_NULL : pointer(u), Float64(dtol), cosatol,
    count, lagsum, csum, ndup, GSS_MEM_HOST, C_NULL))
  abscissa = [c > 0 ? s / c : NaN for (s, c) in zip(lagsum, count)]
  ordinate = [count[k] == 0 ? NaN : csum[k, p] / 2count[k] for k in 1:nlags, p in 1:size(csum, 2)]
  (vars=names, abscissa=abscissa, ordinate=ordinate, counts=count, nduplicates=ndup[])
end

"column of the pair (a, b) of 1-based variable positions in the `ordinate` of `empirical_cross_variogram`"
pairindex(nz::Integer, a::Integer, b::Integer) = (a > b ? pairindex(nz, b, a) : (a - 1) * nz - (a - 1) * (a - 2) ÷ 2 + (b - a) + 1)

"""
    fit_lmc(kinds, cross; weighting=:count, order=1.0)

Linear model of coregionalisation Γ(h) = B0 + B1 f(h / range) fitted to the result of `empirical_cross_variogram`
(gss_variogram_fit_lmc, host code of the library).  Returns `(variograms, correlation, B0, B1, range)`: `variograms[v]`
is the direct model of variable `v` (sill B0_vv + B1_vv, nugget B0_vv, the shared range; the Gaussian nugget rule is that
of `fit_variogram`) and `correlation[(a, b)]` = (B0_ab + B1_ab) / sqrt(sill_a sill_b) is the number the LUGS solver takes as
the joint parameter `correlation` of `(a, b)`.
"""
function fit_lmc(kinds, cross; weighting::Symbol=:count, order::Real=1.0)
  ks = kinds isa Type ? [kinds] : collect(kinds)
  codes = Int32[something(findfirst(==(k), GAMMA_CONSTRUCTORS), 8) - 1 for k in ks]      # anything else: GSS_VG_POWER
  w = weighting == :count ? Int32(0) : weighting == :uniform ? Int32(2) : Int32(1)
  nz = length(cross.vars)
  h = collect(Float64, cross.abscissa)
  gam = Matrix{Float64}(cross.ordinate)             # pair p at gam + (p - 1) * nlags
  cnt = collect(Int64, cross.counts)
  kind = Ref{Int32}(0)
  range = Ref{Float64}(0.0)
  B0 = Matrix{Float64}(undef, nz, nz)
  B1 = Matrix{Float64}(undef, nz, nz)               # symmetric: row-major and column-major agree
  objective = Vector{Float64}(undef, length(codes))
  check(ccall((:gss_variogram_fit_lmc, libgss), Int32,
    (Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Int32, Int32, Ptr{Int32}, Int32, Float64, Int32, Ptr{Int32}, Ptr{Float64},
     Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), h, gam, cnt, Int32(length(cnt)), Int32(nz), codes, Int32(length(codes)),
    Float64(order), w, kind, range, B0, B1, objective))
  T = GAMMA_CONSTRUCTORS[kind[]+1]
  function direct(a)
    sill, nug = B0[a, a] + B1[a, a], B0[a, a]
    nug = T === GaussianVariogram ? max(nug - GAUSSIAN_NUGGET_EPS[], 0.0) : nug
    T === MaternVariogram ? T(sill=sill, nugget=nug, range=range[], order=Float64(order)) : T(sill=sill, nugget=nug, range=range[])
  end
  S = B0 .+ B1
  variograms = Dict(v => direct(a) for (a, v) in enumerate(cross.vars))
  correlation = Dict((cross.vars[a], cross.vars[b]) => S[a, b] / sqrt(S[a, a] * S[b, b]) for a in 1:nz for b in a+1:nz)
  (variograms=variograms, correlation=correlation, B0=B0, B1=B1, range=range[])
end

# ---- several GPUs: one worker process per GPU ---------------------------------------------------------------------
# Everything below runs through remotecall_fetch on workers that have loaded this module and called bind_device.
"""
    bind_device(dev)

Bind this process to GPU `dev` (gss_init): call it once on every worker before a `solve(...; procs=workers())`,
e.g. `@everywhere workers() GeoStatsSolversHIP.bind_device(myid() - 2)`.
"""
bind_device(dev::Integer) = check(ccall((:gss_init, libgss), Int32, (Int32,), Int32(dev)))

const WORKER_STATE = Dict{UInt64,Any}()     # run id => preproc: the device handles stay alive between remote calls

function export_token(kind::Int32, handle::Handle)
  tok = Vector{UInt8}(undef, GSS_IPC_TOKEN_BYTES)
  GC.@preserve tok check(ccall((:gss_state_ipc_export, libgss), Int32, (Int32, Ptr{Cvoid}, Ptr{UInt8}), kind, handle, tok))
  tok
end
function import_token!(kind::Int32, handle::Handle, tok::Vector{UInt8})
  GC.@preserve tok check(ccall((:gss_state_ipc_import, libgss), Int32, (Int32, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Cvoid}),
                               kind, handle, tok, C_NULL))
end

# (key, state kind, handle) of every device state a preprocess holds
statehandles(pre, ::FFTGSHIP) = [(var, GSS_STATE_FFTGS, par.handle) for (var, par) in pre if var !== :_run]
function statehandles(pre, ::LUGSHIP)
  out = Any[]
  for (conames, coparams) in pre
    conames === :_run && continue
    for (key, par) in coparams
      key isa Set && length(key) == 1 && push!(out, ((conames, key), GSS_STATE_LUGS, par.handle))
    end
  end
  out
end
worker_preprocess_impl(problem, solver::FFTGSHIP; kw...) = fftgs_preprocess(problem, solver; kw...)
worker_preprocess_impl(problem, solver::LUGSHIP; kw...) = lugs_preprocess(problem, solver; kw...)
worker_preprocess_impl(problem, solver::SGSHIP; kw...) = sgs_preprocess(problem, solver; kw...)
statehandles(pre, ::SGSHIP) = Any[]          # nothing to move (see sgs_preprocess)

# owner (tokens === nothing): preprocess, return one token per state; peer: create without state, import
function worker_preprocess(id::UInt64, problem, solver, seed::UInt64, tokens)
  pre = worker_preprocess_impl(problem, solver; compute=isnothing(tokens), seed=seed)
  WORKER_STATE[id] = pre
  isnothing(tokens) && return Dict(key => export_token(kind, h) for (key, kind, h) in statehandles(pre, solver))
  for (key, kind, h) in statehandles(pre, solver)
    import_token!(kind, h, tokens[key])
  end
  nothing
end

# realisations first .. first+count-1 of every variable: Dict(var => npts x count)
function worker_block(id::UInt64, problem, solver::FFTGSHIP, first::Int, count::Int)
  pre = WORKER_STATE[id]
  Dict(var => fftgs_block(problem, pre, var, first, count) for covars in covariables(problem, solver) for var in covars.names)
end
function worker_block(id::UInt64, problem, solver::LUGSHIP, first::Int, count::Int)
  pre = WORKER_STATE[id]
  out = Dict{Symbol,Matrix{Float64}}()
  for covars in covariables(problem, solver)
    merge!(out, lugs_block(pre, covars.names, first, count))
  end
  out
end
function worker_block(id::UInt64, problem, solver::SGSHIP, first::Int, count::Int)
  pre = WORKER_STATE[id]
  Dict(var => sgs_block(pre, var, first, count) for covars in covariables(problem, solver) for var in covars.names)
end
function worker_release(id::UInt64, solver)
  pre = pop!(WORKER_STATE, id, nothing)
  isnothing(pre) && return nothing
  if solver isa SGSHIP
    for (var, par) in pre
      var !== :_run && !isnothing(par.shared[]) && destroy!(par.shared[])
    end
  end
  for (_, _, h) in statehandles(pre, solver)
    destroy!(h)
  end
  nothing
end

blockrange(n::Int, i::Int, P::Int) = (q = divrem(n, P); lo = (i - 1) * q[1] + min(i - 1, q[2]); (lo, q[1] + (i <= q[2] ? 1 : 0)))

# estimation: blocks of domain elements; every worker returns its columns in domain order, the visiting order of the
# solver's `path` (krig.jl:179-183) is applied once at the end
linearpath(solver::KrigingSolverHIP, problem) =
  KrigingSolverHIP((Tuple(covars.names) => merge(covars.params[Set(covars.names)], (path=LinearPath(),))
                    for covars in covariables(problem, solver))...)
function worker_points(problem, solver, lo::Int, cnt::Int)
  sub = EstimationProblem(data(problem), view(domain(problem), (lo + 1):(lo + cnt)), Tuple(keys(variables(problem))))
  cols = Tables.columns(values(solve(sub, solver)))
  Dict(name => collect(Tables.getcolumn(cols, name)) for name in Tables.columnnames(cols))
end
function solve_points_on_workers(problem::EstimationProblem, solver::KrigingSolverHIP, procs::Vector{Int})
  pdomain = domain(problem)
  m, P = nelements(pdomain), length(procs)
  lin = linearpath(solver, problem)
  parts = asyncmap(1:P) do i
    lo, cnt = blockrange(m, i, P)
    remotecall_fetch(worker_points, procs[i], problem, lin, lo, cnt)
  end
  cols = Dict(name => reduce(vcat, [part[name] for part in parts]) for name in keys(parts[1]))
  for covars in covariables(problem, solver), var in covars.names
    order = collect(traverse(pdomain, covars.params[Set([var])].path))
    for name in (var, Symbol(var, "_variance"))
      cols[name] = cols[name][order]
    end
  end
  georef((; (name => cols[name] for name in sort(collect(keys(cols)); by=string))...), pdomain)
end

function solve_on_workers(problem::SimulationProblem, solver, procs::Vector{Int})
  seed = rand(solver.rng, UInt64)                  # the reference consumes solver.rng in the same place (fft.jl:147)
  id = rand(UInt64)
  R, P = nreals(problem), length(procs)
  try
    tokens = remotecall_fetch(worker_preprocess, procs[1], id, problem, solver, seed, nothing)   # preprocess ONCE
    @sync for p in procs[2:end]
      @async remotecall_fetch(worker_preprocess, p, id, problem, solver, seed, tokens)
    end
    parts = asyncmap(1:P) do i
      lo, cnt = blockrange(R, i, P)
      remotecall_fetch(worker_block, procs[i], id, problem, solver, lo, cnt)
    end
    reals = Dict{Symbol,Vector{Vector{Float64}}}()
    for var in keys(parts[1])
      reals[var] = [part[var][:, r] for part in parts for r in 1:size(part[var], 2)]
    end
    return ensemble(problem, reals)
  finally
    foreach(p -> remotecall_fetch(worker_release, p, id, solver), procs)
  end
end

# ---- SGS (sgs.jl:45-89 over seq.jl:42-141) -----------------------------------------------------
@simsolver SGSHIP begin
  @param variogram = GaussianVariogram()
  @param mean = 0.0
  @param path = LinearPath()
  @param minneighbors = 1
  @param maxneighbors = 10
  @param neighborhood = nothing
  @param distance = Euclidean()
  @global init = NearestInit()
  @global rng = Random.GLOBAL_RNG      # sgs.jl:54
end

const SGS_PATHS_PER_HANDLE = 64   # visiting orders per device handle when every realisation has its own

preprocess(problem::SimulationProblem, solver::SGSHIP) = sgs_preprocess(problem, solver)

# (no transferable state: the neighbour lists and weights of a visiting order are built where they are used, so on
# several GPUs every worker prepares the orders of its own realisations; `compute` is accepted for symmetry)
function sgs_preprocess(problem::SimulationProblem, solver::SGSHIP; compute=true, seed=nothing)
  pdomain = domain(problem)
  buff, mask = initbuff(pdomain, variables(problem), solver.init, data=data(problem))   # seq.jl:85
  C = coordmatrix(pdomain)
  d, N = size(C)
  preproc = Dict{Any,Any}()
  for covars in covariables(problem, solver), var in covars.names
    p = covars.params[Set([var])]
    metric, _ = searchmetric(p)                                           # seq.jl:91-98; a ball replaces the metric
    # (GSS_METRIC_HAVERSINE runs on the exhaustive search, which the library offers for the mask-after-search reading
    # this shim always passes)
    dlocs = Int64.(findall(mask[var]) .- 1)
    zdata = Float64.(buff[var][mask[var]])
    k = p.maxneighbors
    if k < 1 || k > N                                                     # searcher_ui, ui.jl:18-20
      @warn "Invalid maximum number of neighbors. Adjusting to $N..."
      k = N
    end
    radius, ir = ballspec(p.neighborhood)
    # the device state is built per block of realisations in sgs_block: `traverse` is called once per realisation,
    # as the reference does inside solvesingle (seq.jl:99-102), so a RandomPath gives every realisation its own order
    preproc[var] = (pdomain=pdomain, path=p.path, C=C, N=N, d=d, dlocs=dlocs, zdata=zdata, k=Int32(k),
                    minneighbors=Int32(p.minneighbors), radius=radius, ir=ir, vg=cvariogram(p.variogram, d),
                    mean=Float64(p.mean), metric=metric, shared=Ref{Union{Nothing,Handle}}(nothing))
  end
  preproc[:_run] = RunState(problem, solver; seed)
  preproc
end

function sgs_handle(par, paths::Matrix{Int64}, base::Int)
  vg = Ref(par.vg)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  C, dlocs, zdata, ir = par.C, par.dlocs, par.zdata, par.ir
  GC.@preserve C paths dlocs zdata ir check(ccall((:gss_sgs_create_paths, libgss), Int32,
    (Ptr{Ptr{Cvoid}}, Ptr{GssVariogram}, Float64, Ptr{Float64}, Int64, Int32, Ptr{Int64}, Int64, Int64, Ptr{Int64},
     Ptr{Float64}, Int64, Int32, Int32, Float64, Ptr{Float64}, Int32, Ptr{Cvoid}),
    h, vg, par.mean, C, par.N, Int32(par.d), paths, size(paths, 2), Int64(base), dlocs, zdata, length(dlocs), par.k,
    par.minneighbors, par.radius, ir, GSS_SGS_MASK_AFTER_SEARCH | (par.metric << GSS_SGS_METRIC_SHIFT),
    C_NULL))   # search!(...; mask=simulated): mask after the query; bits 4..6: the search metric
  Handle(h[], :sgs)
end

function sgs_realize!(out, handle, seed, first::Int, count::Int)
  GC.@preserve out check(ccall((:gss_sgs_realize, libgss), Int32,
    (Ptr{Cvoid}, UInt64, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Cvoid}),
    handle, seed, Int64(first), Int64(count), C_NULL, out, GSS_MEM_HOST, C_NULL))
  out
end

# realisations first .. first+count-1 (N x count)
function sgs_block(preproc, var, first::Int, count::Int)
  par = preproc[var]
  seed = varseed(preproc[:_run], var)
  out = Matrix{Float64}(undef, par.N, count)
  count == 0 && return out
  if par.path isa LinearPath                      # the same order for every realisation: one handle, lanes = realisations
    if isnothing(par.shared[])
      par.shared[] = sgs_handle(par, reshape(Int64.(collect(traverse(par.pdomain, par.path)) .- 1), par.N, 1), 0)
    end
    return sgs_realize!(out, par.shared[], seed, first, count)
  end
  for a in first:SGS_PATHS_PER_HANDLE:(first + count - 1)
    b = min(a + SGS_PATHS_PER_HANDLE, first + count)
    paths = reduce(hcat, [Int64.(collect(traverse(par.pdomain, par.path)) .- 1) for _ in a:(b - 1)])   # seq.jl:102
    h = sgs_handle(par, paths, a)
    sgs_realize!(view(out, :, (a - first + 1):(b - first)), h, seed, a, b - a)
    destroy!(h)
  end
  out
end

function solvesingle(::SimulationProblem, covars::NamedTuple, solver::SGSHIP, preproc)
  r = nextreal!(preproc[:_run], covars.names)
  Dict(var => sgs_block(preproc, var, r, 1)[:, 1] for var in covars.names)
end

function solve(problem::SimulationProblem, solver::SGSHIP; procs=[myid()])
  procs == [myid()] || return solve_on_workers(problem, solver, collect(procs))
  preproc = preprocess(problem, solver)
  reals = Dict{Symbol,Vector{Vector{Float64}}}()
  for covars in covariables(problem, solver), var in covars.names
    Z = sgs_block(preproc, var, 0, nreals(problem))
    reals[var] = [Z[:, r] for r in 1:nreals(problem)]
    isnothing(preproc[var].shared[]) || destroy!(preproc[var].shared[])
  end
  ensemble(problem, reals)
end

end # module
