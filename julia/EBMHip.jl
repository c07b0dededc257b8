# EBMHip.jl — Julia shim that routes EnergyBalanceModel.jl's step!/integrate hot path to the
# MI355X library behind include/ebm_hip.h.
#
# NOT EXECUTED IN THIS PIPELINE: no Julia toolchain exists here (SURVEY F3).  It is the binding a
# maintainer of the reference would add; it contains no numerics, only `ccall`s.  The Python
# mirror (energybalancemodel.jl_amd/infrastructure.py) makes the same calls through ctypes and is
# what the tests exercise.
#
# THE supported calls (the same two forms are documented in INTEGRATION.md and include/ebm_hip.h):
#
#   using EnergyBalanceModel, EBMHip
#   sols = EBMHip.integrate(:MIZ, st, forcing, par, init; lastonly=true, verbose=false)
#   EBMHip.step!(Val(:MIZ), t, f, vars, st, par)
#
# i.e. the reference's own signatures (src/infrastructure.jl:615-618, src/miz.jl:150-154,
# src/classic.jl:37-41) and the reference's own model symbols, as functions of THIS module.
# `EBMHip.integrate` keeps the state on the device for the whole run and fills a `Solutions` exactly
# as the reference does; `EBMHip.step!` is the per-call form (five fields up, ten down per call).
#
# Why there is no `:MIZ_HIP` model tag.  Extending the reference's generic `step!` with a
# `Val{:MIZ_HIP}` method would make `EnergyBalanceModel.integrate(:MIZ_HIP, ...)` callable, and that
# call does the wrong thing without failing: the reference's `integrate` only adds the seven MIZ
# variables to the solution when `model === :MIZ` (src/infrastructure.jl:621-624), so E, T, h alone
# would be stored, and `default_parameters(:MIZ_HIP)` returns the CLASSIC parameter set
# (src/infrastructure.jl:473-474).  The reference dispatches on the symbol's VALUE; a new tag cannot
# be made to mean "MIZ".  Hence: same symbols, functions of this module.
module EBMHip

using EnergyBalanceModel
using EnergyBalanceModel.Infrastructure: Vec, Collection, SpaceTime, Forcing, Solutions, default_parval
import EnergyBalanceModel.Infrastructure

const libebm = get(ENV, "EBM_HIP_LIB", "libebm_hip.so")

# enum ebm_param / ebm_field (include/ebm_hip.h)
const PARAM_ORDER = (:D, :A, :B, :cw, :S0, :S1, :S2, :a0, :a2, :ai, :Fb, :k, :Lf, :F, :cg, :tau,
                     :Tm, :m1, :m2, :alpha, :rl, :Dmin, :Dmax, :hmin, :kappa)
const FIELD = Dict(:Ei => 0, :Ew => 1, :h => 2, :D => 3, :phi => 4, :T0 => 5, :Tw => 6, :Ti => 7,
                   :n => 8, :E => 9, :T => 10, :Tg => 11)
const MODEL = Dict(:MIZ => 0, :Classic => 1, :MIZ_IMEX => 2)
# :MIZ_IMEX is NOT a model of the reference: the MIZ model with its meridional diffusion treated implicitly
# (EBM_MODEL_MIZ_IMEX in include/ebm_hip.h), for time steps beyond the explicit limit.  It exists only through
# EBMHip.integrate / EBMHip.step!; pass default_parameters(:MIZ) with it.
ismiz(model::Symbol) = model === :MIZ || model === :MIZ_IMEX

struct EBMError <: Exception
    msg::String
end
check(rc::Cint, what) = rc == 0 ? nothing :
    throw(EBMError("$what failed ($rc): " * unsafe_string(ccall((:ebm_last_error, libebm), Cstring, ()))))

gridkind(::SpaceTime{identity}) = Cint(0)
gridkind(::SpaceTime) = Cint(1)

parvec(par::Collection{Float64}) =
    Float64[haskey(getfield(par, :dict), k) ? getproperty(par, k) : getproperty(default_parval, k) for k in PARAM_ORDER]

# struct ebm_options (include/ebm_hip.h): launch options; the library reads no environment variable.
struct EBMOptions
    struct_bytes::Cint
    cells_per_thread::Cint      # 0 = default (4); 2: twice the waves per meridian, for a few short meridians
    use_graph::Cint             # -1 = by size
    prefetch_cols::Cint         # -1 = default
    launch_chains::Cint         # -1 / 1 = one launch per step; 2 = two independent chains over the two halves of the columns
    integrate_steps_per_launch::Cint   # -1 = 64 steps per launch where integrate needs only the running sums; 1 = every step its own launch
    fused_state_in_lds::Cint    # -1 = by column count; 0 / 1: fused-K launches keep the state in registers / in LDS (same bits)
    elide_zero_lines::Cint      # -1 / 1 = the one-step kernel that derives phi skips state lines that are all zero; 0 = off (same bits)
end
EBMOptions(; cells_per_thread::Integer=0, use_graph::Integer=-1, prefetch_cols::Integer=-1, launch_chains::Integer=-1,
           integrate_steps_per_launch::Integer=-1, fused_state_in_lds::Integer=-1, elide_zero_lines::Integer=-1) =
    EBMOptions(Cint(sizeof(EBMOptions)), Cint(cells_per_thread), Cint(use_graph), Cint(prefetch_cols), Cint(launch_chains),
               Cint(integrate_steps_per_launch), Cint(fused_state_in_lds), Cint(elide_zero_lines))

# One ebm_handle_t.  Every ccall that passes `h.ptr` sits inside `GC.@preserve h`: the pointer alone
# does not keep `h` alive, and its finalizer calls ebm_destroy.
mutable struct Handle
    ptr::Ptr{Cvoid}
    function Handle(model::Symbol, st::SpaceTime, par::Collection{Float64}; ncol::Int=1, device::Int=0,
                    cells_per_thread::Int=(ncol == 1 && st.nx <= 1536 && model !== :MIZ_IMEX) ? 2 : 0)
        haskey(MODEL, model) || throw(MethodError(Infrastructure.step!, (Val(model),)))   # as the reference: no such method
        out = Ref{Ptr{Cvoid}}(C_NULL)
        # The reference's own shapes are ONE meridian: latency-bound, so two latitudes per thread.  Chosen here,
        # explicitly — the library never derives its launch geometry from the number of columns, because the rounding
        # of the tridiagonal solves depends on it (a member must give the same bits alone and in an ensemble).
        opt = Ref(EBMOptions(cells_per_thread=cells_per_thread))
        check(ccall((:ebm_create_ex, libebm), Cint,
                    (Ref{Ptr{Cvoid}}, Cint, Cint, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Cdouble, Cint, Ref{EBMOptions}),
                    out, MODEL[model], gridkind(st), st.nx, ncol, st.x, parvec(par), st.dt, device, opt), "ebm_create_ex")
        h = new(out[])
        finalizer(destroy!, h)
        return h
    end
end
function destroy!(h::Handle)
    if h.ptr != C_NULL
        ccall((:ebm_destroy, libebm), Cint, (Ptr{Cvoid},), h.ptr)
        h.ptr = C_NULL
    end
    return nothing
end

setfield_dev!(h::Handle, f::Symbol, v::Vec) = GC.@preserve h check(
    ccall((:ebm_set_field, libebm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}), h.ptr, FIELD[f], v), "ebm_set_field")
function getfield_dev(h::Handle, f::Symbol, n::Int)::Vec
    v = Vector{Float64}(undef, n)
    GC.@preserve h check(
        ccall((:ebm_get_field, libebm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}), h.ptr, FIELD[f], v), "ebm_get_field")
    return v
end

cos2pit(t::Float64) = cos(2.0*pi * t)              # as written at src/miz.jl:11

# The reference keeps its T0 warm start in a module-level closure (src/miz.jl:47); the mirror of
# that for direct step! calls is one cached handle per (model, grid, parameters).
const _handles = Dict{UInt64,Handle}()
handle_for(model, st, par) = get!(() -> Handle(model, st, par), _handles, hash((model, st.x, st.dt, parvec(par))))

const INIT = Dict(:MIZ => (:Ei, :Ew, :h, :D, :phi), :Classic => (:E, :Tg), :MIZ_IMEX => (:Ei, :Ew, :h, :D, :phi))
const OUT = Dict(:MIZ => (:Ei, :Ew, :h, :D, :phi, :Tw, :Ti, :n, :E, :T), :Classic => (:E, :Tg, :T, :h),
                 :MIZ_IMEX => (:Ei, :Ew, :h, :D, :phi, :Tw, :Ti, :n, :E, :T))

"""
    EBMHip.step!(Val(model), t, f, vars, st, par; debug=nothing, verbose=false) -> vars

The reference's `step!` (`src/miz.jl:150-196`, `src/classic.jl:37-71`) on the GPU: uploads the
prognostic fields of `vars`, takes one step (`ebm_step`), rebinds the fields of `vars` to fresh
vectors as the reference does, returns `vars`.  The hidden T0 warm start persists between calls like
the reference's (one cached handle per model / grid / parameter set).  `debug` expressions are
evaluated inside the reference's step! (`src/miz.jl:188-191`) and cannot cross a C ABI: with
`debug !== nothing` the call is forwarded to the reference's own method.
"""
function step!(::Val{M}, t::Float64, f::Float64, vars::Collection{Vec}, st::SpaceTime, par::Collection{Float64};
               debug::Union{Expr,Nothing}=nothing, verbose::Bool=false) where M
    model = M::Symbol
    if !isnothing(debug)      # the :Classic method has no `verbose` keyword at the reference commit (SURVEY F7)
        model === :MIZ_IMEX && throw(ArgumentError("debug expressions need the reference's step!, which has no :MIZ_IMEX"))
        return model === :MIZ ? Infrastructure.step!(Val(model), t, f, vars, st, par; debug=debug, verbose=verbose) :
                                Infrastructure.step!(Val(model), t, f, vars, st, par; debug=debug)
    end
    h = handle_for(model, st, par)
    foreach(k -> setfield_dev!(h, k, getproperty(vars, k)), INIT[model])
    if ismiz(model)
        ct, ctn = cos2pit(t), 0.0
    else
        i = round(Int, mod1((t + st.dt/2.0) * st.nt, st.nt))          # src/classic.jl:45
        ct, ctn = cos2pit(st.t[i]), cos2pit(st.t[mod1(i+1, st.nt)])
    end
    before = verbose ? counters(h)[3] : 0
    GC.@preserve h check(ccall((:ebm_step, libebm), Cint, (Ptr{Cvoid}, Cdouble, Cdouble, Cdouble, Cint),
                               h.ptr, ct, ctn, f, 1), "ebm_step")
    foreach(k -> setproperty!(vars, k, getfield_dev(h, k, st.nx)), OUT[model])
    verbose && counters(h)[3] > before && @warn "Solving for T0 failed at t=$t."     # src/miz.jl:61-63
    return vars
end

function counters(h::Handle)
    c = zeros(Clonglong, 4)
    GC.@preserve h check(ccall((:ebm_get_counters, libebm), Cint, (Ptr{Cvoid}, Ptr{Clonglong}), h.ptr, c), "ebm_get_counters")
    return c
end

"""
    EBMHip.integrate(model, st, forcing, par, init; lastonly=true, debug=nothing, verbose=false, device=0) -> Solutions

The reference's `integrate` (`src/infrastructure.jl:615-636`) with the state resident on the device
for the whole run: `ebm_integrate` steps `st.nt * st.dur` times and performs `savesol!`
(`:549-591`) and `annual_mean` (`:536-544`) there; the returned `Solutions` holds the same `raw`,
`seasonal.winter / summer / avg` and `ts` as the reference's.  `model` is `:MIZ` or `:Classic`
(the reference's `integrate(:Classic, ...)` throws on its `verbose` keyword at this commit — SURVEY
F7 — this one works and stores E, T, h as `:621` prescribes).  With `debug !== nothing` the call is
forwarded to the reference's own `integrate`.
"""
function integrate(model::Symbol, st::SpaceTime{F}, forcing::Forcing{C}, par::Collection{Float64}, init::Collection{Vec};
                   lastonly::Bool=true, debug::Union{Expr,Nothing}=nothing, verbose::Bool=false,
                   device::Int=0)::Solutions{F,C} where {F, C}
    isnothing(debug) || return Infrastructure.integrate(model, st, forcing, par, init; lastonly=lastonly, debug=debug, verbose=verbose)
    solvars = Set{Symbol}((:E, :T, :h))                                     # src/infrastructure.jl:621-624
    ismiz(model) && union!(solvars, Set{Symbol}((:Ei, :Ew, :Ti, :Tw, :D, :phi, :n)))
    sols = Solutions(st, forcing, par, init, solvars, lastonly)
    names = collect(solvars)
    h = Handle(model, st, par; device=device)          # owns the T0 warm start of this run (re-entrant, unlike src/miz.jl:47)
    try
        foreach(k -> setfield_dev!(h, k, getproperty(init, k)), INIT[model])
        ctab = cos2pit.(st.t)
        fsteps = Float64[forcing(T) for T in st.T]
        nraw, nx, dur = length(sols.ts), st.nx, st.dur
        raw = Array{Float64,3}(undef, nx, nraw, length(names))         # == C [nvars][nraw][1][nlat]
        win, sum_, avg = (Array{Float64,3}(undef, nx, dur, length(names)) for _ in 1:3)
        GC.@preserve h begin
            check(ccall((:ebm_set_time_table, libebm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cdouble}), h.ptr, st.nt, ctab),
                  "ebm_set_time_table")
            check(ccall((:ebm_integrate, libebm), Cint,
                        (Ptr{Cvoid}, Cint, Cint, Ptr{Cdouble}, Cint, Cint, Cint, Cint, Ptr{Cint},
                         Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                        h.ptr, st.nt, dur, fsteps, lastonly, st.winter.inx, st.summer.inx, length(names),
                        Cint[FIELD[k] for k in names], raw, win, sum_, avg), "ebm_integrate")
        end
        for (vi, k) in enumerate(names)
            setproperty!(sols.raw, k, [raw[:, ti, vi] for ti in 1:nraw])
            setproperty!(sols.seasonal.winter, k, [win[:, y, vi] for y in 1:dur])
            setproperty!(sols.seasonal.summer, k, [sum_[:, y, vi] for y in 1:dur])
            setproperty!(sols.seasonal.avg, k, [avg[:, y, vi] for y in 1:dur])
        end
        if verbose
            nfail = counters(h)[3]
            nfail > 0 && @warn "Solving for T0 hit the iteration cap at $nfail time steps."
        end
    finally
        destroy!(h)                                    # explicit: do not wait for the finalizer
    end
    return sols
end

"""
    set_member_forcings!(h, forcings::Vector{<:Forcing})

One `Forcing` per column (ensemble member), evaluated on the device at `st.T[tinx]` of every
step with the reference's own call operator (`src/infrastructure.jl:294-307`).
"""
function set_member_forcings!(h::Handle, forcings::AbstractVector)
    words = Matrix{Float64}(undef, 9, length(forcings))           # column-major == C [ncol][9]
    for (c, f) in enumerate(forcings)
        if f isa Forcing{true}
            words[:, c] = [f.base, f.base, f.base, 0.0, 0.0, Inf, Inf, Inf, Inf]
        else
            words[:, c] = [f.base, f.peak, f.cool, f.rates[1], f.rates[2],
                           Float64(f.domain[2]), Float64(f.domain[3]), Float64(f.domain[4]), Float64(f.domain[5])]
        end
    end
    GC.@preserve h check(ccall((:ebm_set_column_schedule, libebm), Cint, (Ptr{Cvoid}, Ptr{Cdouble}), h.ptr, words),
                         "ebm_set_column_schedule")
end

"""
    run_series!(h, first_step, fsteps, every, names; ncol=1, steps_per_launch=64) -> Array{Float64,3}

`length(fsteps)` steps from 0-based global step `first_step` (time table set beforehand) with the per-column
`hemispheric_mean` (`src/utilities.jl:397-403`) of every variable in `names` sampled on the device after every `every`
steps (`ebm_run_series`): `out[c, j, v]` is column `c`, sample `j`, variable `names[v]`.
"""
function run_series!(h::Handle, first_step::Integer, fsteps::Vector{Float64}, every::Integer, names::Vector{Symbol};
                     ncol::Int=1, steps_per_launch::Integer=64)
    nsteps = length(fsteps)
    (every >= 1 && nsteps % every == 0) || throw(ArgumentError("the number of steps must be a multiple of every >= 1"))
    out = Array{Float64,3}(undef, ncol, div(nsteps, every), length(names))        # == C [nvars][nsamples][ncol]
    GC.@preserve h check(ccall((:ebm_run_series, libebm), Cint,
                               (Ptr{Cvoid}, Clonglong, Cint, Ptr{Cdouble}, Cint, Cint, Cint, Ptr{Cint}, Ptr{Cdouble}),
                               h.ptr, first_step, nsteps, fsteps, every, steps_per_launch, length(names),
                               Cint[FIELD[k] for k in names], out), "ebm_run_series")
    return out
end

"""
    run_until!(h, first_step, fsteps, every, name, level, direction; steps_per_launch=64)
        -> (samples, crossed, value)

First passage (`ebm_run_until`): rounds of `every` steps from 0-based global step `first_step`, at most
`length(fsteps) ÷ every` of them; after each round the per-column `hemispheric_mean` of field `name` is taken on the
device, and a column whose mean has crossed `level[c]` (`direction[c] > 0`: mean >= level, `< 0`: mean <= level; a NaN mean
never crosses) takes no further step.  `samples[c]` rounds were taken by column `c`; its first-passage step is
`first_step + samples[c]*every - 1` where `crossed[c]`; `value[c]` is its last mean.
"""
function run_until!(h::Handle, first_step::Integer, fsteps::Vector{Float64}, every::Integer, name::Symbol,
                    level::Vector{Float64}, direction::Vector{<:Integer}; steps_per_launch::Integer=64)
    nsteps = length(fsteps)
    (every >= 1 && nsteps >= every && nsteps % every == 0) ||
        throw(ArgumentError("the number of steps must be a positive multiple of every >= 1"))
    ncol = length(level)
    length(direction) == ncol || throw(ArgumentError("level and direction must have one entry per column"))
    samples, crossed, value = zeros(Cint, ncol), zeros(Cint, ncol), fill(NaN, ncol)
    GC.@preserve h check(ccall((:ebm_run_until, libebm), Cint,
                               (Ptr{Cvoid}, Clonglong, Cint, Cint, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cint},
                                Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}),
                               h.ptr, first_step, div(nsteps, every), every, fsteps, steps_per_launch, FIELD[name], level,
                               Cint.(sign.(direction)), samples, crossed, value), "ebm_run_until")
    return Int.(samples), crossed .!= 0, value
end

"""
    resample!(h, parents)

Selection step of a cloning / splitting / particle-filter algorithm on the device (`ebm_resample_columns`): for every
column `c` at once (1-based here), the new state of `c` is the old state of column `parents[c]` — prognostic fields, warm
start, noise state and every field that is current.  Column `c` keeps its own forcing offset, schedule, parameter row and
noise stream.  `parents[c] == c` moves nothing; the step clock and the validity of the fields are unchanged.
"""
function resample!(h::Handle, parents::Vector{<:Integer})
    GC.@preserve h check(ccall((:ebm_resample_columns, libebm), Cint, (Ptr{Cvoid}, Ptr{Cint}), h.ptr, Cint.(parents .- 1)),
                         "ebm_resample_columns")
end

"""
    column_record(h) -> (record_doubles, mask)

The doubles of one exported column (`ebm_column_record`: a function of the model, `nlat` and `cells_per_thread` only) and
the mask an export would return now (bit `f`: field `f` is current).
"""
function column_record(h::Handle)
    n, m = Ref{Clonglong}(0), Ref{Cuint}(0)
    GC.@preserve h check(@ccall(libebm.ebm_column_record(h.ptr::Ptr{Cvoid}, n::Ref{Clonglong}, m::Ref{Cuint})::Cint),
                         "ebm_column_record")
    return Int(n[]), m[]
end

"""
    export_columns!(h, cols, devbuf) -> mask
    import_columns!(h, cols, devbuf, mask; records=nothing)

Whole columns (1-based here) into a packed device buffer of records and back (`ebm_export_columns`,
`ebm_import_columns`): record `i` of `devbuf` — a device pointer to `length(cols) * column_record(h)[1]` doubles, 16-byte
aligned — is the state of column `cols[i]`, every field in the natural layout, with the warm start and the noise state;
on import column `cols[i]` (distinct) takes record `records[i]` (default `i`) and keeps its own settings and noise
stream.  Both are asynchronous on the handle's stream; across handles the caller orders the work (see the header).
"""
function export_columns!(h::Handle, cols::Vector{<:Integer}, devbuf::Ptr{Cdouble})
    m = Ref{Cuint}(0)
    c = Cint.(cols .- 1)
    GC.@preserve h check(@ccall(libebm.ebm_export_columns(h.ptr::Ptr{Cvoid}, length(c)::Cint, c::Ptr{Cint}, devbuf::Ptr{Cdouble},
                                                          m::Ref{Cuint})::Cint), "ebm_export_columns")
    return m[]
end

function import_columns!(h::Handle, cols::Vector{<:Integer}, devbuf::Ptr{Cdouble}, mask::Integer; records=nothing)
    c = Cint.(cols .- 1)
    r = records === nothing ? Ptr{Cint}(C_NULL) : Cint.(records .- 1)
    GC.@preserve h check(@ccall(libebm.ebm_import_columns(h.ptr::Ptr{Cvoid}, length(c)::Cint, c::Ptr{Cint}, r::Ptr{Cint},
                                                          devbuf::Ptr{Cdouble}, Cuint(mask)::Cuint)::Cint), "ebm_import_columns")
end

"""
    ensemble_sums(h, names; ncol, nlat, weights=nothing, center=nothing) -> Array{Float64,3}
    ensemble_sums_device!(h, names, devout; weights=nothing, center=nothing)

Weighted sums across the columns, per latitude, reduced on the device (`ebm_ensemble_sums`; the definition is in the
header): `out[k, q, v]` is `S_(q-1)` of variable `names[v]` at latitude `k` — `S0 = sum w`, `S1 = sum w d`,
`S2 = sum (w d) d` with `d = x - center[k, v]` (`d = x` without `center`) over the columns whose weight is not 0 and whose
cell is not NaN.  `weights`: `ncol` values (`nothing`: all 1.0); `center`: `nlat x length(names)`.  The order of the sums is
fixed (blocks of 32 columns), so the bits do not depend on the run, the launch geometry or the layout the handle holds.
The `_device!` form writes the packed array to the device pointer `devout` (the payload of an all-reduce between shards).
"""
function ensemble_sums(h::Handle, names::Vector{Symbol}; ncol::Integer, nlat::Integer, weights=nothing, center=nothing)
    out = Array{Float64,3}(undef, nlat, 3, length(names))
    f = Cint[FIELD[k] for k in names]
    w = weights === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(weights)
    c = center === nothing ? Ptr{Cdouble}(C_NULL) : Matrix{Float64}(center)
    weights === nothing || length(weights) == ncol || error("weights: expected $ncol values")
    center === nothing || size(center) == (nlat, length(names)) || error("center: expected $nlat x $(length(names)) values")
    GC.@preserve h check(@ccall(libebm.ebm_ensemble_sums(h.ptr::Ptr{Cvoid}, length(f)::Cint, f::Ptr{Cint}, w::Ptr{Cdouble},
                                                         c::Ptr{Cdouble}, out::Ptr{Cdouble})::Cint), "ebm_ensemble_sums")
    return out
end

function ensemble_sums_device!(h::Handle, names::Vector{Symbol}, devout::Ptr{Cdouble}; weights=nothing, center=nothing)
    f = Cint[FIELD[k] for k in names]
    w = weights === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(weights)
    c = center === nothing ? Ptr{Cdouble}(C_NULL) : Matrix{Float64}(center)
    GC.@preserve h check(@ccall(libebm.ebm_ensemble_sums_device(h.ptr::Ptr{Cvoid}, length(f)::Cint, f::Ptr{Cint}, w::Ptr{Cdouble},
                                                                c::Ptr{Cdouble}, devout::Ptr{Cdouble})::Cint),
                         "ebm_ensemble_sums_device")
end

"""
    ensemble_covariance(h, name_a, name_b=name_a; ncol, nlat, weights=nothing, center_a=nothing, center_b=nothing) -> Matrix{Float64}
    ensemble_covariance_device!(h, name_a, name_b, devout; weights=nothing, center_a=nothing, center_b=nothing)

Covariance across the columns for every pair of latitudes, reduced on the device with the fp64 matrix instruction
(`ebm_ensemble_covariance`; the definition is in the header): `out[i, j] = sum_c (w_c (x_c[i] - center_a[i])) (y_c[j] -
center_b[j])`, `x` the cells of `name_a` and `y` those of `name_b`; a zero weight removes the member and a NaN cell
contributes nothing.  `weights`: `ncol` values (`nothing`: all 1.0); the centers: `nlat` values each (`nothing`: nothing is
subtracted).  One field against itself about one center gives a matrix that is symmetric to the bit.  The `_device!` form
writes the packed row-major array (`out[i][j]` at `i * nlat + j`, 0-based) to the device pointer `devout`.
"""
function ensemble_covariance(h::Handle, name_a::Symbol, name_b::Symbol=name_a; ncol::Integer, nlat::Integer, weights=nothing,
                             center_a=nothing, center_b=nothing)
    out = Matrix{Float64}(undef, nlat, nlat)
    w = weights === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(weights)
    ca = center_a === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(center_a)
    cb = center_b === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(center_b)
    weights === nothing || length(weights) == ncol || error("weights: expected $ncol values")
    center_a === nothing || length(center_a) == nlat || error("center_a: expected $nlat values")
    center_b === nothing || length(center_b) == nlat || error("center_b: expected $nlat values")
    GC.@preserve h check(@ccall(libebm.ebm_ensemble_covariance(h.ptr::Ptr{Cvoid}, FIELD[name_a]::Cint, FIELD[name_b]::Cint,
                                                               w::Ptr{Cdouble}, ca::Ptr{Cdouble}, cb::Ptr{Cdouble},
                                                               out::Ptr{Cdouble})::Cint), "ebm_ensemble_covariance")
    return permutedims(out)          # the C array is row-major
end

function ensemble_covariance_device!(h::Handle, name_a::Symbol, name_b::Symbol, devout::Ptr{Cdouble}; weights=nothing,
                                     center_a=nothing, center_b=nothing)
    w = weights === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(weights)
    ca = center_a === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(center_a)
    cb = center_b === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(center_b)
    GC.@preserve h check(@ccall(libebm.ebm_ensemble_covariance_device(h.ptr::Ptr{Cvoid}, FIELD[name_a]::Cint, FIELD[name_b]::Cint,
                                                                      w::Ptr{Cdouble}, ca::Ptr{Cdouble}, cb::Ptr{Cdouble},
                                                                      devout::Ptr{Cdouble})::Cint),
                         "ebm_ensemble_covariance_device")
end

"""
    update_columns!(h, names, obs_name, gain, target; nlat, scale=1.0, dev_perturb=C_NULL, lo=nothing, hi=nothing)
    update_columns_device!(h, names, obs_name, dev_gain, target; scale=1.0, dev_perturb=C_NULL, lo=nothing, hi=nothing)

The ensemble Kalman update on the device (`ebm_update_columns`; the definition is in the header): for every prognostic field
`f` of `names`, `x_f[c, k] += sum_j gain[f][k, j] * d[c, j]` with `d[c, j] = (target[j] + e[c, j]) - scale * xo[c, j]`, `xo` the
cell of `obs_name`, on the fp64 matrix instruction.  `gain`: one `nlat x nlat` matrix per field (a vector of matrices, or an
`nlat x nlat x nvars` array indexed `[k, j, v]`); it is passed row-major (`gain[v][k][j]`), as the C array is.  `target`: `nlat`
values, `NaN` where nothing was observed.  `dev_perturb`: a device pointer to `e[ncol][nlat]`, or `C_NULL`.  `lo`, `hi`: one
bound per field, or `nothing`.  The `_device!` form takes the packed gain at a 16-byte aligned device pointer.  Afterwards the
handle is as after `set_field!` of every listed field.
"""
function update_columns!(h::Handle, names, obs_name::Symbol, gain, target; nlat::Integer, scale::Real=1.0,
                         dev_perturb::Ptr{Cdouble}=Ptr{Cdouble}(C_NULL), lo=nothing, hi=nothing)
    f = Cint[FIELD[n] for n in names]
    g = Array{Float64}(undef, nlat, nlat, length(f))          # [j, k, v] column-major = gain[v][k][j] row-major
    for v in eachindex(f)
        gv = gain isa AbstractVector ? gain[v] : view(gain, :, :, v)
        size(gv) == (nlat, nlat) || error("gain: expected $nlat x $nlat per field")
        g[:, :, v] = permutedims(gv)
    end
    y = Vector{Float64}(target)
    length(y) == nlat || error("target: expected $nlat values")
    l = lo === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(lo)
    u = hi === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(hi)
    GC.@preserve h check(@ccall(libebm.ebm_update_columns(h.ptr::Ptr{Cvoid}, length(f)::Cint, f::Ptr{Cint}, FIELD[obs_name]::Cint,
                                                          g::Ptr{Cdouble}, y::Ptr{Cdouble}, Float64(scale)::Cdouble,
                                                          dev_perturb::Ptr{Cdouble}, l::Ptr{Cdouble}, u::Ptr{Cdouble})::Cint),
                         "ebm_update_columns")
end

function update_columns_device!(h::Handle, names, obs_name::Symbol, dev_gain::Ptr{Cdouble}, target; scale::Real=1.0,
                                dev_perturb::Ptr{Cdouble}=Ptr{Cdouble}(C_NULL), lo=nothing, hi=nothing)
    f = Cint[FIELD[n] for n in names]
    y = Vector{Float64}(target)
    l = lo === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(lo)
    u = hi === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(hi)
    GC.@preserve h check(@ccall(libebm.ebm_update_columns_device(h.ptr::Ptr{Cvoid}, length(f)::Cint, f::Ptr{Cint},
                                                                 FIELD[obs_name]::Cint, dev_gain::Ptr{Cdouble}, y::Ptr{Cdouble},
                                                                 Float64(scale)::Cdouble, dev_perturb::Ptr{Cdouble},
                                                                 l::Ptr{Cdouble}, u::Ptr{Cdouble})::Cint),
                         "ebm_update_columns_device")
end

"""
    spd_solve_device!(h, m, nrhs, dev_S, lds, dev_B, ldb) -> info
    kalman_gain_device!(h, obs, obs_var, dev_Poo, dev_Pfo, dev_gain; localize=0.0, factor=1.0) -> info

The Kalman gain on the device (`ebm_spd_solve_device`, `ebm_kalman_gain_device`; the definition is in the header): `X * S = B` for
a symmetric positive definite `S` by a blocked Cholesky factorisation on the fp64 matrix instruction, in place on device
buffers padded to a multiple of 64, and the gain `[nvars][nlat][nlat]` built with it from covariances already on the device.
`obs`: `nlat` values, `NaN` = unobserved; `obs_var`: `nlat` values; `dev_Pfo`: a vector of device pointers, one per field.  A
matrix that is not positive definite raises with the bad pivot in the message.
"""
function spd_solve_device!(h::Handle, m::Integer, nrhs::Integer, dev_S::Ptr{Cdouble}, lds::Integer, dev_B::Ptr{Cdouble}, ldb::Integer)
    info = Ref{Cint}(0)
    GC.@preserve h check(@ccall(libebm.ebm_spd_solve_device(h.ptr::Ptr{Cvoid}, Cint(m)::Cint, Clonglong(nrhs)::Clonglong,
                                                            dev_S::Ptr{Cdouble}, Clonglong(lds)::Clonglong, dev_B::Ptr{Cdouble},
                                                            Clonglong(ldb)::Clonglong, info::Ptr{Cint})::Cint),
                         "ebm_spd_solve_device")
    return Int(info[])
end

function kalman_gain_device!(h::Handle, obs, obs_var, dev_Poo::Ptr{Cdouble}, dev_Pfo::Vector{Ptr{Cdouble}}, dev_gain::Ptr{Cdouble};
                             localize::Real=0.0, factor::Real=1.0)
    y = Vector{Float64}(obs)
    r = Vector{Float64}(obs_var)
    info = Ref{Cint}(0)
    GC.@preserve h check(@ccall(libebm.ebm_kalman_gain_device(h.ptr::Ptr{Cvoid}, length(dev_Pfo)::Cint, y::Ptr{Cdouble}, r::Ptr{Cdouble},
                                                              Float64(localize)::Cdouble, Float64(factor)::Cdouble,
                                                              dev_Poo::Ptr{Cdouble}, dev_Pfo::Ptr{Ptr{Cdouble}}, dev_gain::Ptr{Cdouble},
                                                              info::Ptr{Cint})::Cint),
                         "ebm_kalman_gain_device")
    return Int(info[])
end

"The HIP-event times (ms) of assembly, factor, solves and scatter of the handle's last `kalman_gain_device!` (`ebm_kalman_gain_phases`)."
function kalman_gain_phases(h::Handle)
    ms = zeros(Cfloat, 4)
    GC.@preserve h check(@ccall(libebm.ebm_kalman_gain_phases(h.ptr::Ptr{Cvoid}, ms::Ptr{Cfloat})::Cint), "ebm_kalman_gain_phases")
    return ms
end

"""
    ensemble_range(h, names; ncol, nlat, weights=nothing) -> Array{Float64,3}
    ensemble_range_device!(h, names, devout; weights=nothing)
    ensemble_histogram(h, names, lo, hi, nbins; ncol, nlat, weights=nothing) -> Array{Float64,3}
    ensemble_histogram_device!(h, names, lo, hi, nbins, devout; weights=nothing)

Order statistics across the columns, per latitude, reduced on the device (`ebm_ensemble_range`, `ebm_ensemble_histogram`;
the definitions are in the header).  Range: `out[k, q, v]`, q = 1, 2, 3, is the number of contributing columns of
`names[v]` at latitude `k`, their minimum and their maximum.  Histogram: `out[k, s, v]`, s = 1 ... nbins + 2, the summed
weights below `lo[k, v]`, in the `nbins` bins of `[lo, hi)`, and at or above `hi[k, v]`; `lo`, `hi`: `nlat x length(names)`,
finite, `lo < hi`; `1 <= nbins <= 64`; a name may be repeated, each entry with its own column of edges.  A column
contributes iff its weight is not 0 and its cell is not NaN.  The order of the sums is fixed (blocks of 256 columns); with
`weights === nothing` every slot is an exact count.  The `_device!` forms write the packed array to the device pointer.
"""
function ensemble_range(h::Handle, names::Vector{Symbol}; ncol::Integer, nlat::Integer, weights=nothing)
    out = Array{Float64,3}(undef, nlat, 3, length(names))
    f = Cint[FIELD[k] for k in names]
    w = weights === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(weights)
    weights === nothing || length(weights) == ncol || error("weights: expected $ncol values")
    GC.@preserve h check(@ccall(libebm.ebm_ensemble_range(h.ptr::Ptr{Cvoid}, length(f)::Cint, f::Ptr{Cint}, w::Ptr{Cdouble},
                                                          out::Ptr{Cdouble})::Cint), "ebm_ensemble_range")
    return out
end

function ensemble_range_device!(h::Handle, names::Vector{Symbol}, devout::Ptr{Cdouble}; weights=nothing)
    f = Cint[FIELD[k] for k in names]
    w = weights === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(weights)
    GC.@preserve h check(@ccall(libebm.ebm_ensemble_range_device(h.ptr::Ptr{Cvoid}, length(f)::Cint, f::Ptr{Cint}, w::Ptr{Cdouble},
                                                                 devout::Ptr{Cdouble})::Cint), "ebm_ensemble_range_device")
end

function ensemble_histogram(h::Handle, names::Vector{Symbol}, lo::Matrix{Float64}, hi::Matrix{Float64}, nbins::Integer;
                            ncol::Integer, nlat::Integer, weights=nothing)
    size(lo) == size(hi) == (nlat, length(names)) || error("lo, hi: expected $nlat x $(length(names)) values")
    out = Array{Float64,3}(undef, nlat, nbins + 2, length(names))
    f = Cint[FIELD[k] for k in names]
    w = weights === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(weights)
    weights === nothing || length(weights) == ncol || error("weights: expected $ncol values")
    GC.@preserve h check(@ccall(libebm.ebm_ensemble_histogram(h.ptr::Ptr{Cvoid}, length(f)::Cint, f::Ptr{Cint}, w::Ptr{Cdouble},
                                                              nbins::Cint, lo::Ptr{Cdouble}, hi::Ptr{Cdouble},
                                                              out::Ptr{Cdouble})::Cint), "ebm_ensemble_histogram")
    return out
end

function ensemble_histogram_device!(h::Handle, names::Vector{Symbol}, lo::Matrix{Float64}, hi::Matrix{Float64}, nbins::Integer,
                                    devout::Ptr{Cdouble}; weights=nothing)
    f = Cint[FIELD[k] for k in names]
    w = weights === nothing ? Ptr{Cdouble}(C_NULL) : Vector{Float64}(weights)
    GC.@preserve h check(@ccall(libebm.ebm_ensemble_histogram_device(h.ptr::Ptr{Cvoid}, length(f)::Cint, f::Ptr{Cint},
                                                                     w::Ptr{Cdouble}, nbins::Cint, lo::Ptr{Cdouble},
                                                                     hi::Ptr{Cdouble}, devout::Ptr{Cdouble})::Cint),
                         "ebm_ensemble_histogram_device")
end

"""
    column_misfits(h, names, target; ncol, nlat, rw=nothing) -> Array{Float64,3}
    column_misfits_device!(h, names, target, devout; rw=nothing)

Per-member misfits to target profiles, reduced along each column on the device (`ebm_column_misfits`; the definition is in
the header).  `target`: `nlat x length(names) x ntargets`, finite or NaN ("no observation here"), `1 <= ntargets <= 8`;
`rw`: `nlat x length(names)`, finite and `>= 0`, `nothing` = all 1.  `out[c, 1, t]` = J, the sum over fields and latitudes of
`(rw * d) * d` with `d = x - target`; `out[c, 2, t]` = N, the number of cells that entered it.  A cell contributes iff its
`rw` is not 0 and neither the target nor the cell is NaN.  The order of the adds is fixed.  The `_device!` form writes the
packed array to the device pointer.
"""
function column_misfits(h::Handle, names::Vector{Symbol}, target::Array{Float64,3}; ncol::Integer, nlat::Integer, rw=nothing)
    size(target)[1:2] == (nlat, length(names)) || error("target: expected $nlat x $(length(names)) x ntargets values")
    nt = size(target, 3)
    out = Array{Float64,3}(undef, ncol, 2, nt)
    f = Cint[FIELD[k] for k in names]
    r = rw === nothing ? Ptr{Cdouble}(C_NULL) : Matrix{Float64}(rw)
    rw === nothing || size(rw) == (nlat, length(names)) || error("rw: expected $nlat x $(length(names)) values")
    GC.@preserve h check(@ccall(libebm.ebm_column_misfits(h.ptr::Ptr{Cvoid}, length(f)::Cint, f::Ptr{Cint}, nt::Cint,
                                                          target::Ptr{Cdouble}, r::Ptr{Cdouble}, out::Ptr{Cdouble})::Cint),
                         "ebm_column_misfits")
    return out
end

function column_misfits_device!(h::Handle, names::Vector{Symbol}, target::Array{Float64,3}, devout::Ptr{Cdouble}; rw=nothing)
    f = Cint[FIELD[k] for k in names]
    nt = size(target, 3)
    r = rw === nothing ? Ptr{Cdouble}(C_NULL) : Matrix{Float64}(rw)
    GC.@preserve h check(@ccall(libebm.ebm_column_misfits_device(h.ptr::Ptr{Cvoid}, length(f)::Cint, f::Ptr{Cint}, nt::Cint,
                                                                 target::Ptr{Cdouble}, r::Ptr{Cdouble},
                                                                 devout::Ptr{Cdouble})::Cint), "ebm_column_misfits_device")
end

"""
    column_scalars(h, spec, level; ncol) / column_scalars_device!(h, spec, level, devout)

Column scalars (`ebm_column_scalars`; the definition is in the header): `spec` is `4 x nscal` (`Cint`), column `s` =
`(kind, field, k0, k1)` with `kind` one of `SCALAR_KIND`, `field = FIELD[name]` and `k0 <= k1` the band's first and last cell,
0-based and inclusive; `level[s]` is the level of an edge kind.  `out[c, s]`: the band integral or mean (the sum of
`hemispheric_mean`, in its order), or the interpolated position where the field first reaches the level walking poleward,
`Inf` if it never does.  `run_series_scalars!` and `run_until_scalar!` are `run_series!` and `run_until!` with these scalars
in place of the hemispheric means.
"""
const SCALAR_KIND = Dict(:integral => 0, :mean => 1, :edge_ge => 2, :edge_le => 3)

function column_scalars(h::Handle, spec::Matrix{Cint}, level::Vector{Float64}; ncol::Integer)
    nscal = size(spec, 2)
    (size(spec, 1) == 4 && length(level) == nscal) || error("spec: expected 4 x nscal, level: nscal values")
    out = Matrix{Float64}(undef, ncol, nscal)
    GC.@preserve h check(ccall((:ebm_column_scalars, libebm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}),
                               h.ptr, nscal, spec, level, out), "ebm_column_scalars")
    return out
end

function column_scalars_device!(h::Handle, spec::Matrix{Cint}, level::Vector{Float64}, devout::Ptr{Cdouble})
    GC.@preserve h check(ccall((:ebm_column_scalars_device, libebm), Cint, (Ptr{Cvoid}, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}),
                               h.ptr, size(spec, 2), spec, level, devout), "ebm_column_scalars_device")
end

function run_series_scalars!(h::Handle, first_step::Integer, fsteps::Vector{Float64}, every::Integer, spec::Matrix{Cint},
                             level::Vector{Float64}; ncol::Integer, steps_per_launch::Integer=64)
    nsteps, nscal = length(fsteps), size(spec, 2)
    (every >= 1 && nsteps % every == 0) || throw(ArgumentError("the number of steps must be a multiple of every >= 1"))
    series = Array{Float64,3}(undef, ncol, div(nsteps, every), nscal)
    GC.@preserve h check(ccall((:ebm_run_series_scalars, libebm), Cint,
                               (Ptr{Cvoid}, Clonglong, Cint, Ptr{Cdouble}, Cint, Cint, Cint, Ptr{Cint}, Ptr{Cdouble}, Ptr{Cdouble}),
                               h.ptr, first_step, nsteps, fsteps, every, steps_per_launch, nscal, spec, level, series),
                         "ebm_run_series_scalars")
    return series
end

function run_until_scalar!(h::Handle, first_step::Integer, fsteps::Vector{Float64}, every::Integer, spec::Vector{Cint},
                           scalar_level::Float64, level::Vector{Float64}, direction::Vector{<:Integer};
                           steps_per_launch::Integer=64)
    nsteps = length(fsteps)
    (every >= 1 && nsteps >= every && nsteps % every == 0) ||
        throw(ArgumentError("the number of steps must be a positive multiple of every >= 1"))
    ncol = length(level)
    (length(direction) == ncol && length(spec) == 4) || throw(ArgumentError("level and direction: one entry per column; spec: 4 ints"))
    samples, crossed, value = zeros(Cint, ncol), zeros(Cint, ncol), fill(NaN, ncol)
    GC.@preserve h check(ccall((:ebm_run_until_scalar, libebm), Cint,
                               (Ptr{Cvoid}, Clonglong, Cint, Cint, Ptr{Cdouble}, Cint, Ptr{Cint}, Cdouble, Ptr{Cdouble}, Ptr{Cint},
                                Ptr{Cint}, Ptr{Cint}, Ptr{Cdouble}),
                               h.ptr, first_step, div(nsteps, every), every, fsteps, steps_per_launch, spec, scalar_level, level,
                               Cint.(sign.(direction)), samples, crossed, value), "ebm_run_until_scalar")
    return Int.(samples), crossed .!= 0, value
end

end # module EBMHip
