# BDFHip.jl -- Julia-side binding of libbdf_hip.so (include/bdf.h) for BayesianDataFusion.jl.
#
# UNTESTED IN THIS REPOSITORY: neither the build image nor the GPU box has Julia, and the reference itself is Julia 0.4
# syntax.  This file is written for Julia >= 1.6 and shows the binding a maintainer would add; the same entry points are
# exercised from Python (ctypes) by tests/.  Device buffers are owned through bdf_dev_alloc / bdf_h2d / bdf_d2h.
module BDFHip

using Printf

const lib = get(ENV, "BDF_HIP_LIB", "libbdf_hip.so")

struct BDFError <: Exception
    code::Cint
    msg::String
end

function check(rc::Cint)
    rc == 0 && return nothing
    msg = unsafe_string(ccall((:bdf_last_error, lib), Cstring, ()))
    rc == -1 && throw(ArgumentError(msg))
    rc == -2 && throw(BoundsError(msg))
    throw(BDFError(rc, msg))
end

mutable struct Context
    h::Ptr{Cvoid}
    function Context(device::Integer=0; seed::Integer=0)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:bdf_ctx_create, lib), Cint, (Cint, Ptr{Cvoid}, UInt64, Ref{Ptr{Cvoid}}), device, C_NULL, seed % UInt64, out))
        c = new(out[])
        finalizer(x -> ccall((:bdf_ctx_destroy, lib), Cint, (Ptr{Cvoid},), x.h), c)
        c
    end
    function Context(h::Ptr{Cvoid})                 # a context the library created (bdf_ctx_create_rows / _side)
        c = new(h)
        finalizer(x -> ccall((:bdf_ctx_destroy, lib), Cint, (Ptr{Cvoid},), x.h), c)
        c
    end
end

set_sweep!(c::Context, i) = check(ccall((:bdf_ctx_set_sweep, lib), Cint, (Ptr{Cvoid}, UInt32), c.h, i))
function sync(c::Context)
    check(ccall((:bdf_ctx_sync, lib), Cint, (Ptr{Cvoid},), c.h))
    bits = Ref{UInt32}(0)
    check(ccall((:bdf_ctx_warnings, lib), Cint, (Ptr{Cvoid}, Ref{UInt32}), c.h, bits))
    # BDF_WARN_CG_MAXITER: cg_AtA (parallel_cg.jl:73-93) returns such a column silently
    (bits[] & 0x40) != 0 && @warn "beta update: a conjugate-gradient column was still above its tolerance after maxiter iterations"
    nothing
end
# K1 tuning: rows with more than `item` observations are split into pieces of at most `piece` (defaults 192 / 128)
set_item_size!(c::Context, item) = check(ccall((:bdf_ctx_set_item_size, lib), Cint, (Ptr{Cvoid}, Cint), c.h, item))
function item_size(c::Context)
    out = Ref{Cint}(0)
    check(ccall((:bdf_ctx_item_size, lib), Cint, (Ptr{Cvoid}, Ref{Cint}), c.h, out))
    return Int(out[])
end
"D <= 16: rows of at most `max_obs` observations of an entity with at least `min_rows` rows are sampled four to a wave (0: off)"
set_small_rows!(c::Context, max_obs, min_rows) = check(ccall((:bdf_ctx_set_small_rows, lib), Cint, (Ptr{Cvoid}, Cint, Int64), c.h, max_obs, min_rows))
# rows of few observations by the low-rank sampler (same distribution as sample_user_basic, other values); max_obs = 0: off
set_lowrank!(c::Context, max_obs=-1, min_rows=8192) = check(ccall((:bdf_ctx_set_lowrank, lib), Cint, (Ptr{Cvoid}, Cint, Int64), c.h, max_obs, min_rows))
# 16 < D <= 32, one two-mode relation: the rows four to a wave in the column layout (K1c, k_rows_col.hip), cut into pieces of at most `max_piece`
# observations; 0: off (the wave-per-row kernel), -1: the default again (128, larger for entities of many observations)
set_col_rows!(c::Context, max_piece=-1) = check(ccall((:bdf_ctx_set_col_rows, lib), Cint, (Ptr{Cvoid}, Cint), c.h, max_piece))
# how the latest row launch under `entity_tag` was dispatched: rows by K1-lr, K1s, K1c, K1; K1's items; K1c's waves
function rows_dispatch(c::Context, entity_tag::Integer)
    out = zeros(Int64, 6)
    check(ccall((:bdf_ctx_rows_dispatch, lib), Cint, (Ptr{Cvoid}, UInt32, Ptr{Int64}), c.h, UInt32(entity_tag), out))
    return out
end
# K1c at D = 32 gathers from a lane-ordered image of the opposite sample (k_gather_image.hip): 1 on (the default), 0 off -- the same
# values either way; 2: the full image (measured slower)
set_gather_image!(c::Context, on=1) = check(ccall((:bdf_ctx_set_gather_image, lib), Cint, (Ptr{Cvoid}, Cint), c.h, on))
# K1c launches that gathered from an image, images packed from a sample, launches that left their entity's image
function gather_image_stats(c::Context)
    out = zeros(Int64, 3)
    check(ccall((:bdf_ctx_gather_image_stats, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}), c.h, out))
    return out
end
# parity hooks: the image the context holds of the `rows` rows at the device address `sample` into the host array `out`; the pack
# kernel alone, into device memory
gather_image_read!(c::Context, sample::Ptr{Cvoid}, rows::Integer, out::Array{Float64}) =
    check(ccall((:bdf_ctx_gather_image_read, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}), c.h, sample, rows, out))
gather_image_pack!(c::Context, sample::Ptr{Cvoid}, rows::Integer, image::Ptr{Cvoid}) =
    check(ccall((:bdf_gather_image_pack, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}), c.h, sample, rows, image))
set_piece_size!(c::Context, piece) =check(ccall((:bdf_ctx_set_piece_size, lib), Cint, (Ptr{Cvoid}, Cint), c.h, piece))
# a row context on a library-owned stream that leaves `reserve_cus` CUs (0, 8, 16, ...) free, and side contexts that really
# run beside it -- on the reserved CUs (`reserved = true`: the hyperprior's small kernels) or on the others
function rows_context(device::Integer=0; seed::Integer=0, reserve_cus::Integer=8)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:bdf_ctx_create_rows, lib), Cint, (Cint, UInt64, Cint, Ref{Ptr{Cvoid}}), device, seed % UInt64, reserve_cus, out))
    return Context(out[])
end
function side_context(main::Context; apart::Vector{Context}=Context[], reserved::Bool=false)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    hs = Ptr{Cvoid}[a.h for a in apart]
    check(ccall((:bdf_ctx_create_side, lib), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Cint, Cint, Ref{Ptr{Cvoid}}), main.h, hs, length(hs), reserved, out))
    return Context(out[])
end

"device copy of a Julia array (column-major as is)"
mutable struct DevArray{T}
    ctx::Context
    p::Ptr{Cvoid}
    dims::Tuple
end
function DevArray(c::Context, a::Array{T}) where T
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:bdf_dev_alloc, lib), Cint, (Ptr{Cvoid}, Csize_t, Ref{Ptr{Cvoid}}), c.h, sizeof(a), p))
    check(ccall((:bdf_h2d, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), c.h, p[], a, sizeof(a)))
    d = DevArray{T}(c, p[], size(a))
    finalizer(x -> ccall((:bdf_dev_free, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), x.ctx.h, x.p), d)
    d
end
"(blocks, bytes) of device and pinned host memory that the library's own objects hold in this process"
function dev_live()
    blocks = Ref{Int64}(0); bytes = Ref{Int64}(0)
    check(ccall((:bdf_dev_live, lib), Cint, (Ref{Int64}, Ref{Int64}), blocks, bytes))
    (blocks[], bytes[])
end
function Base.Array(d::DevArray{T}) where T
    a = Array{T}(undef, d.dims...)
    check(ccall((:bdf_d2h, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), d.ctx.h, a, d.p, sizeof(a)))
    a
end

"Relation.data (IndexedDF / FastIDF) on the device: replaces FastIDF(rel.data) + @spawnat (src/macau.jl:50-52)"
mutable struct DevRelation
    h::Ptr{Cvoid}
    ctx::Context                      # keeps the context alive for as long as the relation (the library frees through it)
    function DevRelation(c::Context, ids::Matrix{Int64}, values::Vector{Float64}, dims::Vector{Int64})
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:bdf_relation_create, lib), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Ptr{Cvoid}, Cint, Ptr{Float64}, Ref{Ptr{Cvoid}}),
                    c.h, size(ids, 2), dims, size(ids, 1), ids, 8, values, out))
        r = new(out[], c)
        finalizer(x -> ccall((:bdf_relation_destroy, lib), Cint, (Ptr{Cvoid},), x.h), r)
        r
    end
    """
    Several GPUs: the relation of rank `rank` of `world` -- the full IndexedDF index, but on the device only the observations
    of the rows this rank owns, at the internal positions `pos[m]` (0-based, from `layout`) of every mode (bdf_relation_create_sharded).
    """
    function DevRelation(c::Context, ids::Matrix{Int64}, values::Vector{Float64}, dims::Vector{Int64},
                         pos::Vector{Vector{Int32}}, cmax::Vector{Int64}, rank::Integer, world::Integer, chunks::Integer)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        pp = Ptr{Int32}[pointer(p) for p in pos]
        GC.@preserve pos check(ccall((:bdf_relation_create_sharded, lib), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Ptr{Int32}}, Ptr{Int64}, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
                    c.h, size(ids, 2), dims, size(ids, 1), ids, 8, values, pp, cmax, rank, world, chunks, out))
        r = new(out[], c)
        finalizer(x -> ccall((:bdf_relation_destroy, lib), Cint, (Ptr{Cvoid},), x.h), r)
        r
    end
end

# struct bdf_term of include/bdf.h (BDF_MAX_MODES = 4)
struct Term
    rel::Ptr{Cvoid}
    mode::Int32
    _pad::Int32
    alpha::Float64
    mean_value::Float64
    linear_values::Ptr{Cvoid}
    factors::NTuple{4,Ptr{Cvoid}}
    alpha_dev::Ptr{Cvoid}             # C_NULL, or rel.model.alpha in device memory (sampled there: sample_alpha inside sweep!)
    obs_precision::Ptr{Cvoid}         # C_NULL, or a precision weight per observation in COO order (known weights; robust_draw!'s omega)
end

"""
    sample_rows!(ctx, D, N, terms, mu, Lambda, entity_tag, out; shard=0, n_shards=1)

Replaces `sample_latent_all2!` (src/sampling.jl:149-172) and `sample_user2_all!` (:251-264): every row of the entity
(or the rows of one shard) is drawn into the device sample matrix `out` (D x N).
"""
function sample_rows!(c::Context, D, N, terms::Vector{Term}, mu::DevArray{Float64}, Lambda::DevArray{Float64}, entity_tag,
                      out::DevArray{Float64}; shard=0, n_shards=1, prior_pack=nothing)
    check(ccall((:bdf_sample_rows, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Cint, Ptr{Term}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, UInt32, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, D, N, length(terms), terms, mu.p, length(mu.dims) == 2 ? 1 : 0, Lambda.p, entity_tag, shard, n_shards, out.p,
                prior_pack === nothing ? C_NULL : prior_pack.p))
end

"""
    sample_rows_spike!(ctx, D, N, terms, spike_state, u_current, entity_tag, out; shard=0, n_shards=1)

The rows of an entity with the spike-and-slab prior (the reference has none): u_id = s_id w_id, one coordinate after the other from
the exact conditional of (s_id, w_id), starting from the row's current value `u_current` (D x N); `spike_state` holds pi, tau,
logit pi and log tau (4 D doubles).
"""
function sample_rows_spike!(c::Context, D, N, terms::Vector{Term}, spike_state::DevArray{Float64}, u_current::DevArray{Float64}, entity_tag,
                            out::DevArray{Float64}; shard=0, n_shards=1)
    check(ccall((:bdf_sample_rows_spike, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Cint, Ptr{Term}, Ptr{Cvoid}, Ptr{Cvoid}, UInt32, Cint, Cint, Ptr{Cvoid}),
                c.h, D, N, length(terms), terms, spike_state.p, u_current.p, entity_tag, shard, n_shards, out.p))
end

"the spike-and-slab prior's hyper step: pi_d ~ Beta(incl_a + n_d, incl_b + N - n_d), tau_d ~ Gamma(shape + n_d / 2, rate + q_d / 2) into spike_state"
function spike_hyper!(c::Context, D, N, sample::DevArray{Float64}, incl_a, incl_b, shape, rate, entity_tag, spike_state::DevArray{Float64})
    check(ccall((:bdf_spike_hyper, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Float64, Float64, Float64, Float64, UInt32, Ptr{Cvoid}),
                c.h, D, N, sample.p, incl_a, incl_b, shape, rate, entity_tag, spike_state.p))
end

"one retained draw into the running sums of the spike-and-slab result: row_sum (D x N) += [u != 0]; hyper_sum (3 D) += pi, tau, n_d"
function spike_accumulate!(c::Context, D, N, sample::DevArray{Float64}, spike_state::DevArray{Float64}, row_sum::DevArray{Float64},
                           hyper_sum::DevArray{Float64})
    check(ccall((:bdf_spike_accumulate, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, D, N, sample.p, spike_state.p, row_sum.p, hyper_sum.p))
end

"""
    sample_rows_nonneg!(ctx, D, N, terms, tau, u_current, entity_tag, out; shard=0, n_shards=1)

The rows of an entity with the non-negative prior (the reference has none): u_id ~ N(0, 1 / tau_d) truncated to u_id >= 0, one
coordinate after the other from its truncated-normal conditional by inversion, starting from the row's current value `u_current`
(D x N); `tau` holds the D precisions.
"""
function sample_rows_nonneg!(c::Context, D, N, terms::Vector{Term}, tau::DevArray{Float64}, u_current::DevArray{Float64}, entity_tag,
                             out::DevArray{Float64}; shard=0, n_shards=1)
    check(ccall((:bdf_sample_rows_nonneg, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Cint, Ptr{Term}, Ptr{Cvoid}, Ptr{Cvoid}, UInt32, Cint, Cint, Ptr{Cvoid}),
                c.h, D, N, length(terms), terms, tau.p, u_current.p, entity_tag, shard, n_shards, out.p))
end

"parity hook: the non-negative prior's coordinate sweep alone on given systems P (D x D x n_rows), c (D x n_rows); system i is that of row row_begin + i"
function nonneg_sweep!(c::Context, D, n_rows, P::DevArray{Float64}, cvec::DevArray{Float64}, u_current::DevArray{Float64}, entity_tag, row_begin,
                       out::DevArray{Float64})
    check(ccall((:bdf_nonneg_sweep, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, UInt32, Int64, Ptr{Cvoid}),
                c.h, D, n_rows, P.p, cvec.p, u_current.p, entity_tag, row_begin, out.p))
end

"the non-negative prior's hyper step: tau_d ~ Gamma(shape + N / 2, rate + q_d / 2) into tau"
function nonneg_hyper!(c::Context, D, N, sample::DevArray{Float64}, shape, rate, entity_tag, tau::DevArray{Float64})
    check(ccall((:bdf_nonneg_hyper, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Float64, Float64, UInt32, Ptr{Cvoid}),
                c.h, D, N, sample.p, shape, rate, entity_tag, tau.p))
end

"one retained draw into the running sums of the non-negative result: row_sum (D x N) += u; hyper_sum (D) += tau"
function nonneg_accumulate!(c::Context, D, N, sample::DevArray{Float64}, tau::DevArray{Float64}, row_sum::DevArray{Float64},
                            hyper_sum::DevArray{Float64})
    check(ccall((:bdf_nonneg_accumulate, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, D, N, sample.p, tau.p, row_sum.p, hyper_sum.p))
end

"rows per chunk of the non-negative prior's launches on this context; 0: the default"
set_nonneg_chunk!(c::Context, rows) = check(ccall((:bdf_ctx_set_nonneg_chunk, lib), Cint, (Ptr{Cvoid}, Int64), c.h, rows))

"ConditionalNormalWishart + rand (src/sampling.jl:116-127, src/normal_wishart.jl:38-42; call site src/macau.jl:120-134)"
function update_prior!(c::Context, D, N, sample, uhat, sumU, UUt, mu0, b0, Tinv, nu, entity_tag, mu, Lambda;
                       prior_pack=nothing, draws=nothing)   # prior_pack: bdf_prior_pack_doubles(D) doubles; draws: bdf_hyper_draws
    check(ccall((:bdf_hyper_sums, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, D, N, sample.p, uhat === nothing ? C_NULL : uhat.p, sumU.p, UUt.p))
    check(ccall((:bdf_hyper_sample, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ptr{Cvoid}, Float64, UInt32, Ptr{Cvoid}, Ptr{Cvoid},
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, D, N, sumU.p, UUt.p, mu0.p, b0, Tinv.p, nu, entity_tag, mu.p, Lambda.p, C_NULL,
                prior_pack === nothing ? C_NULL : prior_pack.p, draws === nothing ? C_NULL : draws.p))
end

"update_beta! (src/sampling.jl:361-370): feat is a bdf_feat handle from bdf_feat_create_{dense,csr,bin}"
function update_beta!(c::Context, feat::Ptr{Cvoid}, D, sample, mu, Lambda, lambda_beta_dev, use_ff::Bool, tol, sample_lambda::Bool,
                      nu, mu_h, entity_tag, beta)
    check(ccall((:bdf_sample_beta, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Float64, Cint, Cint, Float64, Float64,
                 UInt32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, feat, D, sample.p, mu.p, Lambda.p, lambda_beta_dev.p, use_ff, tol, 0, sample_lambda, nu, mu_h, entity_tag,
                beta.p, C_NULL, C_NULL))
end

# ---- Entity.F operators (S4: F*B, At_mul_B(F,B); RelationData.jl:314-329) ----------------------------------------------
"dense feature matrix (N x numF, column-major as a Julia Matrix{Float64})"
function feat_dense(c::Context, F::Matrix{Float64})
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:bdf_feat_create_dense, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}),
                c.h, size(F, 1), size(F, 2), F, out))
    out[]
end
"sparse features from 1-based COO rows/cols (Int32) and values; `vals === nothing`: binary (SparseBinMatrix / SparseBinMatrixCSR)"
function feat_sparse(c::Context, m, n, rows::Vector{Int32}, cols::Vector{Int32}, vals=nothing)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    if vals === nothing
        check(ccall((:bdf_feat_create_bin, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int32}, Ptr{Int32}, Ref{Ptr{Cvoid}}),
                    c.h, m, n, length(rows), rows, cols, out))
    else
        check(ccall((:bdf_feat_create_csr, lib), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Ref{Ptr{Cvoid}}),
                    c.h, m, n, length(rows), rows, cols, convert(Vector{Float64}, vals), out))
    end
    out[]
end
feat_destroy(f::Ptr{Cvoid}) = check(ccall((:bdf_feat_destroy, lib), Cint, (Ptr{Cvoid},), f))
"out = F * B (transpose = false) or F' * B; B, out: device, column-major with `ncol` columns"
feat_mul!(c::Context, f::Ptr{Cvoid}, B::DevArray, ncol, out::DevArray; transpose=false) =
    check(ccall((:bdf_feat_mul, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint), c.h, f, B.p, ncol, out.p, transpose))
"uhat = (F beta)' and mu .+ uhat (F_mul_beta, RelationData.jl:314-320; macau.jl:103-104)"
uhat!(c::Context, f::Ptr{Cvoid}, D, beta::DevArray, mu::DevArray, uhat::DevArray, mu_matrix::DevArray) =
    check(ccall((:bdf_uhat, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, f, D, beta.p, mu.p, uhat.p, mu_matrix.p))
"T^-1 += beta' beta * lambda_beta (macau.jl:124-129)"
hyper_feature_terms!(c::Context, D, numF, beta::DevArray, WI::DevArray, lambda_beta::DevArray, Tinv::DevArray) =
    check(ccall((:bdf_hyper_feature_terms, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, D, numF, beta.p, WI.p, lambda_beta.p, Tinv.p))

# ---- test-set prediction (pred(rel, test_vec, F) + running mean; src/sampling.jl:9-45, src/macau.jl:142-203) ----------
mutable struct DevPairs
    h::Ptr{Cvoid}
    n::Int
    function DevPairs(c::Context, ids::Matrix{Int64}, values::Vector{Float64})
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:bdf_pairs_create, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Cint, Ptr{Float64}, Ref{Ptr{Cvoid}}),
                    c.h, size(ids, 2), size(ids, 1), ids, 8, values, out))
        p = new(out[], size(ids, 1))
        finalizer(x -> ccall((:bdf_pairs_destroy, lib), Cint, (Ptr{Cvoid},), x.h), p)
        p
    end
end
"running posterior mean / sum of squares / clamped errors / class hits; stats: DevArray of 4 doubles"
function predict_update!(c::Context, p::DevPairs, D, factors::Vector{<:DevArray}, mean_value, phase, clamp_lo, clamp_hi, class_cut, stats::DevArray)
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_predict_update, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Cint, Float64, Float64, Float64, Ptr{Cvoid}),
                c.h, p.h, D, fp, mean_value, phase, clamp_lo, clamp_hi, class_cut, stats.p))
end

# ---- relation model (src/macau.jl:83-92) ------------------------------------------------------------------------------
"alpha = sample_alpha(alpha_lambda0, alpha_nu0, err) (src/sampling.jl:129-134); stats from predict_sse!, alpha_out: 1 double"
function sample_alpha!(c::Context, p::DevPairs, D, factors::Vector{<:DevArray}, mean_value, lambda0, nu0, rel_tag, stats::DevArray, alpha_out::DevArray)
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_predict_sse, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, p.h, D, fp, mean_value, C_NULL, stats.p))
    check(ccall((:bdf_sample_alpha, lib), Cint, (Ptr{Cvoid}, Float64, Float64, Int64, Ptr{Cvoid}, UInt32, Ptr{Cvoid}),
                c.h, lambda0, nu0, p.n, stats.p + 8, rel_tag, alpha_out.p))
end
"beta = sample_beta_rel(r); linear_values = mean_value + F beta (src/sampling.jl:322-337, src/macau.jl:89-92)"
function sample_beta_rel!(c::Context, f::Ptr{Cvoid}, train::DevPairs, D, factors::Vector{<:DevArray}, mean_value, alpha, lambda_beta,
                          rel_tag, beta::DevArray, linear_values::DevArray)
    fp = Ptr{Cvoid}[x.p for x in factors]
    check(ccall((:bdf_sample_beta_rel, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Float64, Float64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, f, train.h, D, fp, mean_value, alpha, lambda_beta, rel_tag, beta.p, linear_values.p, C_NULL))
end

# ---- the whole iteration (src/macau.jl:80-203 without side information) and the multi-GPU exchange ------------------------
struct GibbsTerm
    rel::Ptr{Cvoid}
    mode::Int32
    entity_of_mode::NTuple{4,Int32}
    alpha::Float64
    mean_value::Float64
end

struct GibbsEntity                                # bdf_gibbs_entity, field for field
    N::Int64
    n_real::Int64
    tag::UInt32
    n_terms::Int32
    terms::NTuple{4,GibbsTerm}
    sample::NTuple{3,Ptr{Cvoid}}
    mu::Ptr{Cvoid}; Lambda::Ptr{Cvoid}; mu0::Ptr{Cvoid}; WI::Ptr{Cvoid}; sumU::Ptr{Cvoid}; UUt::Ptr{Cvoid}
    params::Ptr{Cvoid}; prior_pack::Ptr{Cvoid}; draws::Ptr{Cvoid}
    b0::Float64
    nu0::Float64
    # side information of the entity (Entity.F): C_NULL / zeros = none.  With it the iteration runs F_mul_beta and the per-row
    # prior means before the rows (macau.jl:103-104), the feature terms of the hyperprior (:124-129) and update_beta! (:138-140)
    feat::Ptr{Cvoid}
    beta::Ptr{Cvoid}; uhat::Ptr{Cvoid}; mu_matrix::Ptr{Cvoid}; Tinv::Ptr{Cvoid}; lambda_beta::Ptr{Cvoid}; cg_iters::Ptr{Cvoid}
    use_ff::Int32; sample_lambda_beta::Int32; full_lambda_u::Int32; _pad::Int32
    tol::Float64; lb_nu::Float64; lb_mu::Float64
    # a relation of the entity has background cells (GibbsRelation.bg_weight; C_NULL: none): what background_prior! writes before
    # the entity's rows -- D x D; D (D x N with side information); prior_pack_doubles(D); BDF_MAX_TERMS doubles
    bg_Lambda::Ptr{Cvoid}; bg_mu::Ptr{Cvoid}; bg_pack::Ptr{Cvoid}; bg_alpha_rows::Ptr{Cvoid}
    # the spike-and-slab prior in place of the Normal-Wishart one (spike = 0: none): incl_a, incl_b, shape, rate of spike_hyper! and the
    # state (4 D doubles: pi, tau, logit pi, log tau).  No side information, no background on the entity's relations, one rank
    spike::Int32; _pad_spike::Int32
    spike_a::Float64; spike_b::Float64; spike_shape::Float64; spike_rate::Float64
    spike_state::Ptr{Cvoid}
    # the non-negative prior in place of the Normal-Wishart one (nonneg = 0: none): shape, rate of nonneg_hyper! and tau (D doubles).
    # Not with the spike-and-slab prior, side information or a background / dense relation; one rank
    nonneg::Int32; _pad_nonneg::Int32
    nonneg_shape::Float64; nonneg_rate::Float64
    nonneg_tau::Ptr{Cvoid}
end

mutable struct Gibbs
    h::Ptr{Cvoid}
    # what the native object dereferences for as long as it lives: its row context (bdf_gibbs_sweep / _destroy synchronise
    # its stream) and, once set, the communicator -- held here so that the GC cannot finalize them first
    rows::Context
    comm::Any
    keep::Vector{Any}                 # device arrays and relations the entity descriptions point into
    function Gibbs(rows::Context, num_latent::Integer, entities::Vector{GibbsEntity}; keep::Vector=Any[])
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:bdf_gibbs_create, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{GibbsEntity}, Ref{Ptr{Cvoid}}),
                    rows.h, num_latent, length(entities), entities, out))
        g = new(out[], rows, nothing, collect(Any, keep))
        finalizer(x -> ccall((:bdf_gibbs_destroy, lib), Cint, (Ptr{Cvoid},), x.h), g)
        g
    end
end
"set-up: full iterations for about `ms` milliseconds whose results are discarded -- the chain's state is put back bit for bit, only the
buffers have rotated (ask `current_buffer`) -- to bring the device to its working state (bdf_gibbs_warm_device)"
warm_device!(g::Gibbs, ms::Real) = check(ccall((:bdf_gibbs_warm_device, lib), Cint, (Ptr{Cvoid}, Float64), g.h, ms))
"the host has written `entity`'s sample itself, with nothing of the chain in flight: K1c's gather image of it is packed anew
(bdf_gibbs_sample_written)"
sample_written!(g::Gibbs, entity::Integer) = check(ccall((:bdf_gibbs_sample_written, lib), Cint, (Ptr{Cvoid}, Cint), g.h, entity))

"one Gibbs iteration; phase: 0 burn-in, 1 first posterior sample, 2 later ones, -1 no prediction update"
sweep!(g::Gibbs, i::Integer, phase::Integer=-1) = check(ccall((:bdf_gibbs_sweep, lib), Cint, (Ptr{Cvoid}, UInt32, Cint), g.h, i, phase))
sync(g::Gibbs) = check(ccall((:bdf_gibbs_sync, lib), Cint, (Ptr{Cvoid},), g.h))
function current_buffer(g::Gibbs, entity::Integer)
    b = Ref{Cint}(0)
    check(ccall((:bdf_gibbs_current, lib), Cint, (Ptr{Cvoid}, Cint, Ref{Cint}), g.h, entity - 1, b))
    return b[] + 1
end
"""the iteration piece by piece, for a host that keeps the schedule itself (the prediction update through the entry points above):
what the registered relations' models run before the rows, then one entity's rows -- uhat, the prior with the background and dense
terms folded in, the row launch, with a communicator the exchange -- the data-independent part of its hyperprior draw, its
hyperprior step (`draws_prepared`: `step_draws!` has run under this iteration number) and, with side information, its beta: the
pieces `sweep!` composes, with plain stream order, under the iteration number set with `set_sweep!` on the row and the hyperprior
context.  `pack_valid`: the entity's latest `step_hyper!` has left its prior pack"""
step_relations!(g::Gibbs) = check(ccall((:bdf_gibbs_step_relations, lib), Cint, (Ptr{Cvoid},), g.h))
step_rows!(g::Gibbs, entity::Integer, pack_valid::Bool) =
    check(ccall((:bdf_gibbs_step_rows, lib), Cint, (Ptr{Cvoid}, Cint, Cint), g.h, entity - 1, pack_valid))
step_draws!(g::Gibbs, entity::Integer) = check(ccall((:bdf_gibbs_step_draws, lib), Cint, (Ptr{Cvoid}, Cint), g.h, entity - 1))
step_hyper!(g::Gibbs, entity::Integer, draws_prepared::Bool) =
    check(ccall((:bdf_gibbs_step_hyper, lib), Cint, (Ptr{Cvoid}, Cint, Cint), g.h, entity - 1, draws_prepared))
step_beta!(g::Gibbs, entity::Integer) = check(ccall((:bdf_gibbs_step_beta, lib), Cint, (Ptr{Cvoid}, Cint), g.h, entity - 1))
"parity hook: the `n_terms` terms the entity's next row launch would take, the factors at the current samples"
function row_terms(g::Gibbs, entity::Integer, n_terms::Integer)
    terms = Vector{Term}(undef, n_terms)
    check(ccall((:bdf_gibbs_terms, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Term}), g.h, entity - 1, terms))
    return terms
end
"parity hook: enqueues the fold of the entity's background and dense terms -> device pointers (mu, mu_is_matrix, Lambda, pack or C_NULL)"
function row_prior!(g::Gibbs, entity::Integer, pack_valid::Bool)
    mu = Ref{Ptr{Cvoid}}(C_NULL); Lambda = Ref{Ptr{Cvoid}}(C_NULL); pack = Ref{Ptr{Cvoid}}(C_NULL); is_matrix = Ref{Cint}(0)
    check(ccall((:bdf_gibbs_row_prior, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{Ptr{Cvoid}}, Ref{Cint}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}),
                g.h, entity - 1, pack_valid, mu, is_matrix, Lambda, pack))
    return mu[], is_matrix[] != 0, Lambda[], pack[]
end
set_test!(g::Gibbs, pairs::Ptr{Cvoid}, entity_of_mode::Vector{Int32}, mean_value, clamp_lo, clamp_hi, class_cut, stats::DevArray) =
    check(ccall((:bdf_gibbs_set_test, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Float64, Float64, Float64, Float64, Ptr{Cvoid}),
                g.h, pairs, entity_of_mode, mean_value, clamp_lo, clamp_hi, class_cut, stats.p))

"internal row positions of an entity shared by `world` GPUs (bdf_layout_build): (pos::Vector{Int32} 0-based, cmax)"
function layout(degree::Vector{Int64}, world::Integer, chunks::Integer)
    pos = zeros(Int32, length(degree)); cmax = Ref{Int64}(0)
    check(ccall((:bdf_layout_build, lib), Cint, (Int64, Ptr{Int64}, Cint, Cint, Ptr{Int32}, Ref{Int64}),
                length(degree), degree, world, chunks, pos, cmax))
    return pos, cmax[]
end

"rank 0: the 128-byte RCCL id to hand to the other workers (e.g. with remotecall_fetch)"
function comm_unique_id()
    id = zeros(UInt8, 128)
    check(ccall((:bdf_comm_unique_id, lib), Cint, (Ptr{UInt8},), id))
    return id
end

mutable struct Comm
    h::Ptr{Cvoid}
    ctx::Context                      # bdf_comm_destroy uses the context's device
    function Comm(c::Context, rank::Integer, world::Integer, id::Vector{UInt8})
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:bdf_comm_create, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}, Ref{Ptr{Cvoid}}), c.h, rank, world, id, out))
        m = new(out[], c)
        finalizer(x -> ccall((:bdf_comm_destroy, lib), Cint, (Ptr{Cvoid},), x.h), m)
        m
    end
end
function set_comm!(g::Gibbs, m::Comm)
    check(ccall((:bdf_gibbs_set_comm, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), g.h, m.h))
    g.comm = m                        # the native object keeps the pointer: keep the communicator alive with it
    nothing
end
"""large exchanges by direct all-pairs copies over IPC mappings (bdf_comm_enable_peer).  `fn`: a `@cfunction` pointer to the host's
all-gather, `(user::Ptr{Cvoid}, send::Ptr{Cvoid}, recv::Ptr{Cvoid}, bytes::Csize_t) -> Cint` (e.g. a remotecall round over the
workers): it carries the control messages and orders the copies"""
enable_peer!(m::Comm, fn::Ptr{Cvoid}, user::Ptr{Cvoid}=C_NULL, min_bytes::Integer=4 << 20) =
    check(ccall((:bdf_comm_enable_peer, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), m.h, fn, user, min_bytes))
disable_peer!(m::Comm) = check(ccall((:bdf_comm_disable_peer, lib), Cint, (Ptr{Cvoid},), m.h))
"(collective) one exchange by peer copies whatever its size, complete on return: `buf` (device) holds world blocks of `bytes`, this rank's filled in"
peer_selftest!(c::Context, m::Comm, buf::Ptr{Cvoid}, bytes::Integer) =
    check(ccall((:bdf_comm_peer_selftest, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), c.h, m.h, buf, bytes))
function peer_stats(m::Comm)
    n = Ref{Int64}(0); b = Ref{Int64}(0)
    check(ccall((:bdf_comm_peer_stats, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), m.h, n, b))
    return n[], b[]
end
"in-place exchange of chunk `chunk` (0-based) of the D x N sample matrix between the ranks, then `allgather_join!` (bdf_allgather_rows / _join)"
allgather_rows!(c::Context, m::Comm, D, N, sample::DevArray, chunk::Integer, chunks::Integer) =
    check(ccall((:bdf_allgather_rows, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Cint, Cint), c.h, m.h, D, N, sample.p, chunk, chunks))
allgather_join!(c::Context, m::Comm) = check(ccall((:bdf_allgather_join, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), c.h, m.h))
"update_beta! on several ranks: the conjugate-gradient columns shared out and all-gathered (parallel_matrix.jl:488-507; bdf_sample_beta_ranks)"
function update_beta!(c::Context, m::Comm, feat::Ptr{Cvoid}, D, sample, mu, Lambda, lambda_beta_dev, use_ff::Bool, tol, sample_lambda::Bool,
                      nu, mu_h, entity_tag, beta)
    check(ccall((:bdf_sample_beta_ranks, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Float64, Cint, Cint, Float64, Float64,
                 UInt32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, m.h, feat, D, sample.p, mu.p, Lambda.p, lambda_beta_dev.p, use_ff, tol, 0, sample_lambda, nu, mu_h, entity_tag,
                beta.p, C_NULL, C_NULL))
end

"the relation model on several ranks (rank r holds the block of observations first_obs+1 : first_obs+train.n -- f: those rows of the
relation's feature matrix, train: the same observations as pairs): the squared-error sum is added up over the ranks in rank order
(bdf_sum_ranks) before sample_alpha; n_total: the relation's observations"
function sample_alpha!(c::Context, m::Comm, p::DevPairs, n_total::Integer, D, factors::Vector{<:DevArray}, mean_value, lambda0, nu0, rel_tag,
                       stats::DevArray, alpha_out::DevArray)
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_predict_sse, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, p.h, D, fp, mean_value, C_NULL, stats.p))
    check(ccall((:bdf_sum_ranks, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64), c.h, m.h, stats.p + 8, 1))
    check(ccall((:bdf_sample_alpha, lib), Cint, (Ptr{Cvoid}, Float64, Float64, Int64, Ptr{Cvoid}, UInt32, Ptr{Cvoid}),
                c.h, lambda0, nu0, n_total, stats.p + 8, rel_tag, alpha_out.p))
end
"sample_beta_rel on several ranks (bdf_sample_beta_rel_ranks): F'v and, once, F'F summed over the ranks, the same beta on every rank;
linear_values: world blocks of `block` values, this rank's block written, then gathered in place (bdf_allgather_block)"
function sample_beta_rel!(c::Context, m::Comm, f::Ptr{Cvoid}, train::DevPairs, first_obs::Integer, block::Integer, D, factors::Vector{<:DevArray},
                          mean_value, alpha, lambda_beta, rel_tag, beta::DevArray, linear_values::DevArray)
    fp = Ptr{Cvoid}[x.p for x in factors]
    check(ccall((:bdf_sample_beta_rel_ranks, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint, Ptr{Ptr{Cvoid}}, Float64, Float64, Float64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, m.h, f, train.h, first_obs, D, fp, mean_value, alpha, lambda_beta, rel_tag, beta.p, linear_values.p + 8 * first_obs, C_NULL))
    check(ccall((:bdf_allgather_block, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), c.h, m.h, linear_values.p, 8 * block))
    allgather_join!(c, m)
end

# ---- IndexedDF index, launch order, value mean (a1; src/IndexedDF.jl:10-21, 26, 41-43) ----------------------------------------
"IndexedDF.index on the host, without a device: per mode (rowptr[dims[m]+1] 0-based offsets, rowids[nnz] 1-based COO row numbers)"
function index_build(ids::Matrix{Int64}, dims::Vector{Int64})
    nnz, nm = size(ids)
    rp = [zeros(Int64, d + 1) for d in dims]; ri = [zeros(Int64, max(nnz, 1)) for _ in dims]
    rpp = Ptr{Int64}[pointer(x) for x in rp]; rip = Ptr{Int64}[pointer(x) for x in ri]
    GC.@preserve rp ri check(ccall((:bdf_index_build, lib), Cint, (Cint, Ptr{Int64}, Int64, Ptr{Cvoid}, Cint, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}),
                                   nm, dims, nnz, ids, 8, rpp, rip))
    return [(rp[m], ri[m][1:nnz]) for m in 1:nm]
end
"the device relation's own index of `mode` (1-based mode): getData / getCount / getI (IndexedDF.jl:41-43, 67-70)"
function relation_index(r::DevRelation, mode::Integer, dim::Integer, nnz::Integer)
    rp = Ref{Ptr{Int64}}(C_NULL); ri = Ref{Ptr{Int64}}(C_NULL)
    check(ccall((:bdf_relation_index, lib), Cint, (Ptr{Cvoid}, Cint, Ref{Ptr{Int64}}, Ref{Ptr{Int64}}), r.h, mode - 1, rp, ri))
    return copy(unsafe_wrap(Array, rp[], dim + 1)), copy(unsafe_wrap(Array, ri[], nnz))
end
function relation_value_mean(r::DevRelation)            # valueMean (IndexedDF.jl:26)
    m = Ref{Float64}(0.0)
    check(ccall((:bdf_relation_value_mean, lib), Cint, (Ptr{Cvoid}, Ref{Float64}), r.h, m))
    return m[]
end
"rows of `mode` (1-based) by falling number of observations: the order the row kernel deals its shards from (sampling.jl:154)"
function relation_order(r::DevRelation, mode::Integer, dim::Integer)
    o = zeros(Int32, dim)
    check(ccall((:bdf_relation_order, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Int32}), r.h, mode - 1, o))
    return o .+ Int32(1)
end

# ---- Block / sample_users_blocked (src/sampling.jl:236-249) ---------------------------------------------------------------
"the users of a Block share one covariance: vx (device Int32, 0-based item ids), Yma (device nv x nu), factor (device D x M) -> out (device D x nu)"
sample_block!(c::Context, D, nu, nv, vx::DevArray{Int32}, Yma::DevArray{Float64}, factor::DevArray{Float64}, alpha, mu::DevArray{Float64},
              Lambda::DevArray{Float64}, entity_tag, out::DevArray{Float64}) =
    check(ccall((:bdf_sample_block, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ptr{Cvoid}, Ptr{Cvoid}, UInt32, Ptr{Cvoid}),
                c.h, D, nu, nv, vx.p, Yma.p, factor.p, alpha, mu.p, Lambda.p, entity_tag, out.p))

# ---- prediction (src/sampling.jl:9-45) --------------------------------------------------------------------------------------
"pred(r, probe_vec): udot over the pairs + mean_value (or the pairs' baseline, set_baseline!) -> out (device, one double per pair)"
function predict!(c::Context, p::DevPairs, D, factors::Vector{<:DevArray}, mean_value, out::DevArray{Float64})
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_predict, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Ptr{Cvoid}), c.h, p.h, D, fp, mean_value, out.p))
end
"pred_all(r) (sampling.jl:91-97): every cell of the relation, the last mode fastest -> out (device, prod(dims) doubles)"
function predict_all!(c::Context, dims::Vector{Int64}, D, factors::Vector{<:DevArray}, mean_value, out::DevArray{Float64})
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_predict_all, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Int64}, Cint, Ptr{Ptr{Cvoid}}, Float64, Ptr{Cvoid}),
                c.h, length(dims), dims, D, fp, mean_value, out.p))
end
"per-pair baseline replacing mean_value: mean_value + F_test beta of pred(r, probe_vec, F) (sampling.jl:9-14); `nothing` clears it"
set_baseline!(p::DevPairs, baseline) =
    check(ccall((:bdf_pairs_set_baseline, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), p.h, baseline === nothing ? C_NULL : baseline.p))
"link 0: predictions are udot + base (the default); 1: the probit link, probabilities Phi(udot + base)"
set_link!(p::DevPairs, link::Integer) = check(ccall((:bdf_pairs_set_link, lib), Cint, (Ptr{Cvoid}, Cint), p.h, link))
"probit noise model of a 0/1 relation: the latent z of every observation of `train` (caller's order) given the factors, from the
uniform of stream (12, 0x800000 | rel_tag, observation); linear_out = value - z is what the rows take as linear_values with
alpha = 1; z_out may be `nothing`"
function probit_draw!(c::Context, train::DevPairs, D, factors::Vector{<:DevArray}, mean_value, rel_tag, linear_out::DevArray{Float64}, z_out=nothing)
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_probit_draw, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, train.h, D, fp, mean_value, rel_tag, linear_out.p, z_out === nothing ? C_NULL : z_out.p))
end
"censored (Tobit) noise model of a Gaussian relation: `censor` (device Int8, the caller's order) flags observation k of `train` as
a measurement (0), a lower bound (+1) or an upper bound (-1); the latent z of every flagged observation given the factors, from
the uniform of stream (13, 0x800000 | rel_tag, observation); `alpha_dev` (a device scalar or `nothing`) wins over `alpha`;
linear_out = mean_value + value - z is what the rows take as linear_values with the relation's alpha; z_out may be `nothing`"
function censored_draw!(c::Context, train::DevPairs, censor::DevArray{Int8}, D, factors::Vector{<:DevArray}, mean_value, alpha, alpha_dev,
                        rel_tag, linear_out::DevArray{Float64}, z_out=nothing)
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_censored_draw, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Float64, Ptr{Cvoid}, UInt32, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, train.h, censor.p, D, fp, mean_value, alpha, alpha_dev === nothing ? C_NULL : alpha_dev.p, rel_tag, linear_out.p,
                z_out === nothing ? C_NULL : z_out.p))
end
"interval-censored noise model of a Gaussian relation: `bounds` (device Float64, 2 x n: column k holds the (lower, upper) bounds
of observation k of `train` in the caller's order, either may be infinite; lower == upper: a measurement); the latent z of every
bounded observation given the factors, from the uniform of stream (14, 0x800000 | rel_tag, observation); `alpha_dev` (a device
scalar or `nothing`) wins over `alpha`; linear_out = mean_value + value - z is what the rows take as linear_values with the
relation's alpha; z_out may be `nothing`"
function interval_draw!(c::Context, train::DevPairs, bounds::DevArray{Float64}, D, factors::Vector{<:DevArray}, mean_value, alpha, alpha_dev,
                        rel_tag, linear_out::DevArray{Float64}, z_out=nothing)
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_interval_draw, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Float64, Ptr{Cvoid}, UInt32, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, train.h, bounds.p, D, fp, mean_value, alpha, alpha_dev === nothing ? C_NULL : alpha_dev.p, rel_tag, linear_out.p,
                z_out === nothing ? C_NULL : z_out.p))
end
"robust (Student-t) noise model of a Gaussian relation: the precision weight omega of every observation of `train` given the
factors, omega = 2 G / (nu + alpha e^2) with e = value - mean_value - udot and G ~ Gamma((nu + 1) / 2, 1) from the streams
(16 / 17, 0x800000 | rel_tag, observation); nu >= 1; `alpha_dev` (a device scalar or `nothing`) wins over `alpha`; precision_out
is what the rows take as Term.obs_precision; wsse_out (one device Float64 or `nothing`): sum omega e^2 in a fixed order, what
sample_alpha! takes in place of the sum of squares"
function robust_draw!(c::Context, train::DevPairs, D, factors::Vector{<:DevArray}, mean_value, alpha, alpha_dev, nu, rel_tag,
                      precision_out::DevArray{Float64}, wsse_out=nothing)
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_robust_draw, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Float64, Ptr{Cvoid}, Float64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, train.h, D, fp, mean_value, alpha, alpha_dev === nothing ? C_NULL : alpha_dev.p, nu, rel_tag, precision_out.p,
                wsse_out === nothing ? C_NULL : wsse_out.p))
end
"Polya-Gamma noise models (model 1: logit for 0/1 values; 2: negative-binomial counts with the integer dispersion r >= 1): for every
observation of `train`, psi = udot + mean_value, omega ~ PG(b, psi) from ONE cursor over the blocks of the stream (18, 0x800000 |
rel_tag, observation); precision_out = omega is what the rows take as Term.obs_precision, linear_out = mean_value + value - kappa /
omega as Term.linear_values, with alpha = 1 (b = 1, kappa = value - 1/2; b = value + r, kappa = (value - r) / 2)"
function pg_draw!(c::Context, train::DevPairs, D, factors::Vector{<:DevArray}, mean_value, model, r, rel_tag,
                  precision_out::DevArray{Float64}, linear_out::DevArray{Float64})
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_pg_draw, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Cint, Float64, UInt32, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, train.h, D, fp, mean_value, model, r, rel_tag, precision_out.p, linear_out.p))
end
"a noise precision per row of one entity of a Gaussian relation: for every row j of mode `mode` (0-based) of `rel`, tau_j = G /
(rate + alpha S_j / 2) with S_j the sum of (value - (udot + mean_value))^2 over the row's n_j cells, in a fixed order, and G ~
Gamma(shape + n_j / 2, 1) from the streams (19 / 20, 0x800000 | rel_tag, row j); `train` holds the relation's own cells in its
order; `alpha_dev` (a device scalar or `nothing`) wins over `alpha`; tau_out has one Float64 per row of the mode, precision_out one
per cell (tau of the cell's row: what the rows take as Term.obs_precision); wsse_out (one device Float64 or `nothing`): sum tau_j
S_j in a fixed order, what sample_alpha! takes in place of the sum of squares"
function entity_noise_draw!(c::Context, rel::DevRelation, mode, train::DevPairs, D, factors::Vector{<:DevArray}, mean_value, alpha, alpha_dev,
                            shape, rate, rel_tag, tau_out::DevArray{Float64}, precision_out::DevArray{Float64}, wsse_out=nothing)
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_entity_noise_draw, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Float64, Ptr{Cvoid}, Float64, Float64, UInt32,
                 Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, rel.h, mode, train.h, D, fp, mean_value, alpha, alpha_dev === nothing ? C_NULL : alpha_dev.p, shape, rate, rel_tag,
                tau_out.p, precision_out.p, wsse_out === nothing ? C_NULL : wsse_out.p))
end
struct BiasTerm                                   # bdf_bias_term, field for field
    mode::Int32                                   # the biased mode, 0-based
    _pad::Int32
    shape::Float64                                # lambda ~ Gamma(shape, rate) a priori
    rate::Float64
    bias::Ptr{Cvoid}                              # device Float64 per row of that mode: the last draw
    lambda::Ptr{Cvoid}                            # device Float64: the mode's precision, the last draw (the caller starts it)
end
BiasTerm(mode::Integer, shape, rate, bias::DevArray{Float64}, lambda::DevArray{Float64}) =
    BiasTerm(Int32(mode), Int32(0), Float64(shape), Float64(rate), bias.p, lambda.p)
"row and column biases of a Gaussian relation: one Gibbs step on the biases b^m_j of every listed mode m of `rel` (rising) and on
their precisions lambda_m: e = value - (udot + mean_value) into resid_scratch (one Float64 per cell), per mode and row the sum of e
less the other biased modes' current biases in a fixed order, b^m_j = alpha S_j / prec_j + z_j / sqrt(prec_j) with prec_j =
lambda_m + alpha n_j and z_j normal m of stream (28, 0x800000 | rel_tag, row j), then lambda_m = G / (rate + sum b^2 / 2), G ~
Gamma(shape + N_m / 2, 1) from the streams (29 / 30, 0x800000 | rel_tag, row m); linear_out (one Float64 per cell, the caller's
order) = mean_value + the cell's biases: what the rows take as Term.linear_values and the training pairs as their baseline;
`train` holds the relation's own cells in its order; `alpha_dev` (a device scalar or `nothing`) wins over `alpha`"
function bias_draw!(c::Context, rel::DevRelation, train::DevPairs, D, factors::Vector{<:DevArray}, mean_value, alpha, alpha_dev, rel_tag,
                    terms::Vector{BiasTerm}, resid_scratch::DevArray{Float64}, linear_out::DevArray{Float64})
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_bias_draw, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Float64, Ptr{Cvoid}, UInt32, Cint, Ptr{BiasTerm},
                 Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, rel.h, train.h, D, fp, mean_value, alpha, alpha_dev === nothing ? C_NULL : alpha_dev.p, rel_tag, length(terms), terms,
                resid_scratch.p, linear_out.p))
end
"out (one device Float64 per pair, the caller's order) = mean_value + the biases of every pair, added in rising mode order: the
baseline of test pairs or probe cells over the same entities (of a term only mode and bias are read)"
bias_baseline!(c::Context, pairs::DevPairs, terms::Vector{BiasTerm}, mean_value, out::DevArray{Float64}) =
    check(ccall((:bdf_bias_baseline, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{BiasTerm}, Float64, Ptr{Cvoid}),
                c.h, pairs.h, length(terms), terms, mean_value, out.p))
"pairs_lpd_update! scores pair k with alpha tau[its id in mode `mode` (0-based)]: tau, one device Float64 per row of that mode, is
borrowed and read at every update (keep it alive); `nothing` clears it"
pairs_set_precision_scale!(p::DevPairs, tau, mode::Integer=0) =
    check(ccall((:bdf_pairs_set_precision_scale, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint), p.h, tau === nothing ? C_NULL : tau.p, mode))
"predictions of the pairs become the logistic probability 1 / (1 + exp(-(udot + base))) (link 2)"
pairs_set_logistic_link!(p::DevPairs) = check(ccall((:bdf_pairs_set_logistic_link, lib), Cint, (Ptr{Cvoid},), p.h))
"predictions of the pairs become r exp(min(udot + base, 700)), the mean of the count model (link 3)"
pairs_set_count_link!(p::DevPairs, r) = check(ccall((:bdf_pairs_set_count_link, lib), Cint, (Ptr{Cvoid}, Float64), p.h, r))
"out (one device Float64) = sum over the pairs of weights[k] (value - mean_value - udot)^2, in a fixed order: sample_alpha!'s
sum of squares for a relation with known observation weights"
function pairs_weighted_sse!(c::Context, p::DevPairs, D, factors::Vector{<:DevArray}, mean_value, weights::DevArray{Float64},
                             out::DevArray{Float64})
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_pairs_weighted_sse, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, p.h, D, fp, mean_value, weights.p, out.p))
end
# ---- background cells: implicit feedback (bdf_background_prior, bdf_background_sse; DESIGN.md section 20) ---------------------
struct BackgroundTerm                             # bdf_background_term, field for field
    sum::Ptr{Cvoid}                               # device D: the sum of the other entity's rows (update_prior!'s sumU)
    gram::Ptr{Cvoid}                              # device D x D: their Gram matrix (its UUt)
    alpha::Float64
    alpha_dev::Ptr{Cvoid}                         # C_NULL: `alpha`
    weight::Float64                               # c0
    resid::Float64                                # background value - mean_value
end
"the prior the rows of an entity with background relations are sampled with: Lambda_out = Lambda + sum alpha c0 G, mu_out =
Lambda_out^-1 (Lambda mu + sum alpha c0 rb s) (D, or D x N with mu_is_matrix), their prior pack (shared mean only) and alpha (1 - c0)"
function background_prior!(c::Context, D, N, bg::Vector{BackgroundTerm}, mu::DevArray{Float64}, mu_is_matrix::Bool, Lambda::DevArray{Float64},
                           Lambda_out::DevArray{Float64}, mu_out::DevArray{Float64}, alpha_rows::DevArray{Float64}; prior_pack=nothing)
    check(ccall((:bdf_background_prior, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Cint, Ptr{BackgroundTerm}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, D, N, length(bg), bg, mu.p, mu_is_matrix ? 1 : 0, Lambda.p, Lambda_out.p, mu_out.p,
                prior_pack === nothing ? C_NULL : prior_pack.p, alpha_rows.p))
end
"out[1] = the sum of c e^2 over all N M cells of a background relation, from its listed cells (`weights`: omega_k, nothing: 1) and the
two entities' sums and Gram matrices: sample_alpha!'s sum of squares with n = N M"
function background_sse!(c::Context, p::DevPairs, D, factors::Vector{<:DevArray}, mean_value, weights, value, weight,
                         sumU::DevArray{Float64}, gramU::DevArray{Float64}, sumV::DevArray{Float64}, gramV::DevArray{Float64}, N, M,
                         out::DevArray{Float64})
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_background_sse, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Ptr{Cvoid}, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid},
                 Int64, Int64, Ptr{Cvoid}),
                c.h, p.h, D, fp, mean_value, weights === nothing ? C_NULL : weights.p, value, weight, sumU.p, gramU.p, sumV.p, gramV.p, N, M, out.p))
end
# ---- dense relations (bdf_dense_product, bdf_dense_prior, bdf_dense_sse; DESIGN.md section 25) --------------------------------
"out = R F (N x D), or R' F (M x D) with transpose, for the N x M row-major device matrix R of a dense relation, on the f64 matrix cores"
function dense_product!(c::Context, R::DevArray{Float64}, N, M, D, F::DevArray{Float64}, transpose::Bool, out::DevArray{Float64})
    check(ccall((:bdf_dense_product, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint, Ptr{Cvoid}, Cint, Ptr{Cvoid}),
                c.h, R.p, N, M, D, F.p, transpose ? 1 : 0, out.p))
end
struct DenseTerm                                  # bdf_dense_term, field for field
    gram::Ptr{Cvoid}                              # device D x D: the Gram matrix of the other entity's rows
    C::Ptr{Cvoid}                                 # device N x D: a dense term's rows of R V; C_NULL: a background term
    sum::Ptr{Cvoid}                               # device D: a background term's sum of the other entity's rows; C_NULL: a dense term
    alpha::Float64
    alpha_dev::Ptr{Cvoid}                         # C_NULL: `alpha`
    weight::Float64                               # 1, or the background's c0
    resid::Float64                                # the background's value - mean_value
end
"the prior the rows of an entity with dense relations are sampled with: Lambda_out = Lambda + sum alpha G, mu_out (always D x N) =
Lambda_out^-1 (Lambda mu_i + sum alpha C_i); background terms of the same entity are folded in as background_prior! folds them"
function dense_prior!(c::Context, D, N, terms::Vector{DenseTerm}, mu::DevArray{Float64}, mu_is_matrix::Bool, Lambda::DevArray{Float64},
                      Lambda_out::DevArray{Float64}, mu_out::DevArray{Float64}, alpha_rows::DevArray{Float64})
    check(ccall((:bdf_dense_prior, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Cint, Ptr{DenseTerm}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, D, N, length(terms), terms, mu.p, mu_is_matrix ? 1 : 0, Lambda.p, Lambda_out.p, mu_out.p, alpha_rows.p))
end
"out[1] = the sum of (r - u.v)^2 over all N M cells of a dense relation from C = R V, the two Gram matrices and the sum of r^2 (the
listed cells' as a number, the holes' where dense_impute! left it, nothing: no holes)"
function dense_sse!(c::Context, D, N, U::DevArray{Float64}, C::DevArray{Float64}, gramU::DevArray{Float64}, gramV::DevArray{Float64},
                    sum_r2, holes_r2, out::DevArray{Float64})
    check(ccall((:bdf_dense_sse, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, D, N, U.p, C.p, gramU.p, gramV.p, sum_r2, holes_r2 === nothing ? C_NULL : holes_r2.p, out.p))
end
"the holes of a dense relation (its cells that are not listed, as pairs) drawn from their conditional into R: u.v + z / sqrt(alpha);
stats[1] = the sum of their squares"
function dense_impute!(c::Context, holes::DevPairs, D, factors::Vector{<:DevArray}, alpha, alpha_dev, rel_tag, R::DevArray{Float64}, N, M,
                       stats::DevArray{Float64})
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_dense_impute, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Ptr{Cvoid}, UInt32, Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}),
                c.h, holes.h, D, fp, alpha, alpha_dev === nothing ? C_NULL : alpha_dev.p, rel_tag, R.p, N, M, stats.p))
end
# ---- top-K lists per row from the posterior mean score (bdf_scores_*; DESIGN.md section 21) ------------------------------------
"the sum of u.v over the pushed draws for n_rows scored rows of the first entity against the M rows of the second, a ring of `batch`
draws that are not in the sum yet; rows: device Int32 0-based rows of U (nothing: the rows 0 .. n_rows - 1)"
mutable struct Scores
    h::Ptr{Cvoid}
    ctx::Context
    n_rows::Int
    M::Int
    function Scores(c::Context, n_rows::Integer, M::Integer, D::Integer, batch::Integer=8, rows=nothing)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:bdf_scores_create, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Cint, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
                    c.h, n_rows, M, D, batch, rows === nothing ? C_NULL : rows.p, out))
        s = new(out[], c, n_rows, M)
        finalizer(x -> ccall((:bdf_scores_destroy, lib), Cint, (Ptr{Cvoid},), x.h), s)
        s
    end
end
"this draw's factors (N x D and M x D, row-major) into the ring; a full ring is added into the sum"
scores_push!(s::Scores, U::DevArray{Float64}, V::DevArray{Float64}) =
    check(ccall((:bdf_scores_push, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), s.h, U.p, V.p))
"the buffered draws into the sum (f64 matrix instructions; the sum's bits do not depend on where the flushes fall)"
scores_flush!(s::Scores) = check(ccall((:bdf_scores_flush, lib), Cint, (Ptr{Cvoid},), s.h))
"per scored row the K best columns by sum / draws + mean_value (falling score, equal scores by rising column), the columns listed in
`rel` (a two-mode DevRelation's handle, C_NULL: none) left out; items: device Int32 n_rows x K, 1-based, 0 padding; scores: NaN there"
scores_topk!(s::Scores, rel::Ptr{Cvoid}, K::Integer, mean_value, items::DevArray{Int32}, scores::DevArray{Float64}) =
    check(ccall((:bdf_scores_topk, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Float64, Ptr{Cvoid}, Ptr{Cvoid}), s.h, rel, K, mean_value, items.p, scores.p))
"out (device, 4 Float64) = recall@K, NDCG@K, hit rate and the count of scored rows with a held-out cell above class_cut"
scores_metrics!(s::Scores, items::DevArray{Int32}, K::Integer, test::DevPairs, class_cut, out::DevArray{Float64}) =
    check(ccall((:bdf_scores_metrics, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Float64, Ptr{Cvoid}), s.h, items.p, K, test.h, class_cut, out.p))
"parity hooks: `count` doubles between the sum (from cell `first`) and buf, into the sum when write; the count of draws scores are divided by"
scores_copy!(s::Scores, buf::DevArray{Float64}, first::Integer, count::Integer, write::Bool=false) =
    check(ccall((:bdf_scores_copy, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Cint), s.h, buf.p, first, count, write ? 1 : 0))
scores_set_draws!(s::Scores, draws::Real) = check(ccall((:bdf_scores_set_draws, lib), Cint, (Ptr{Cvoid}, Float64), s.h, draws))
# ---- acquisition lists per row from the moments of u.v over the draws (bdf_acquire_*; DESIGN.md section 30) ---------------------
"the running mean and sum of squared deviations (Welford) of u.v over the pushed draws for n_rows scored rows of the first entity
against the M rows of the second and, with want_prob, the sum of Phi(sqrt(alpha_b) (u.v + mean_value - threshold)); a ring of `batch`
draws that are not in the planes yet.  rows: 0-based rows of U (device Int32) or nothing"
mutable struct Acquire
    h::Ptr{Cvoid}
    ctx::Context
    n_rows::Int
    M::Int
    function Acquire(c::Context, n_rows::Integer, M::Integer, D::Integer, batch::Integer, rows::Union{DevArray{Int32},Nothing}=nothing;
                     want_prob::Bool=false, mean_value::Real=0.0, threshold::Real=0.0)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:bdf_acquire_create, lib), Cint, (Ptr{Cvoid}, Int64, Int64, Cint, Cint, Ptr{Cvoid}, Cint, Float64, Float64, Ref{Ptr{Cvoid}}),
                    c.h, n_rows, M, D, batch, rows === nothing ? C_NULL : rows.p, want_prob ? 1 : 0, mean_value, threshold, out))
        a = new(out[], c, n_rows, M)
        finalizer(x -> ccall((:bdf_acquire_destroy, lib), Cint, (Ptr{Cvoid},), x.h), a)
        a
    end
end
"this draw's factors and its precision into the ring (alpha_dev, a device Float64, wins over alpha); a full ring is folded into the planes"
acquire_push!(a::Acquire, U::DevArray{Float64}, V::DevArray{Float64}, alpha::Real, alpha_dev::Union{DevArray{Float64},Nothing}=nothing) =
    check(ccall((:bdf_acquire_push, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ptr{Cvoid}), a.h, U.p, V.p, alpha,
                alpha_dev === nothing ? C_NULL : alpha_dev.p))
"the buffered draws into the planes (f64 matrix instructions; the planes' bits do not depend on where the flushes fall)"
acquire_flush!(a::Acquire) = check(ccall((:bdf_acquire_flush, lib), Cint, (Ptr{Cvoid},), a.h))
"per scored row the K best columns by rule 0 (ucb: m + kappa sd), 1 (sd) or 2 (prob_above), ordered and padded as scores_topk!'s lists;
mean, sd, prob (device Float64 n_rows x K, or C_NULL): the moments at the listed items"
acquire_topk!(a::Acquire, rel::Ptr{Cvoid}, K::Integer, rule::Integer, kappa::Real, items::DevArray{Int32}, scores::DevArray{Float64},
              mean::Ptr{Cvoid}=C_NULL, sd::Ptr{Cvoid}=C_NULL, prob::Ptr{Cvoid}=C_NULL) =
    check(ccall((:bdf_acquire_topk, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Cint, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                a.h, rel, K, rule, kappa, items.p, scores.p, mean, sd, prob))
"parity hooks: `count` doubles between plane 0 (mean), 1 (M2), 2 (psum) or 3 (score), from cell `first`, and buf; the count of draws"
acquire_copy!(a::Acquire, plane::Integer, buf::DevArray{Float64}, first::Integer, count::Integer, write::Bool=false) =
    check(ccall((:bdf_acquire_copy, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Cvoid}, Int64, Int64, Cint), a.h, plane, buf.p, first, count, write ? 1 : 0))
acquire_set_draws!(a::Acquire, draws::Real) = check(ccall((:bdf_acquire_set_draws, lib), Cint, (Ptr{Cvoid}, Float64), a.h, draws))
# ---- convergence diagnostics of held-out predictions (bdf_diag_*; DESIGN.md section 32) ----------------------------------------
"every pushed draw of the predictions of n_cells pairs and of n_scalars scalars (0, 1: the draw's sum of squared errors, 2: and its
alpha) in one plane of capacity x (n_cells + n_scalars) Float64, draw-major, the cells in the pairs' storage order"
mutable struct Diag
    h::Ptr{Cvoid}
    ctx::Context
    n_cells::Int
    n_scalars::Int
    function Diag(c::Context, n_cells::Integer, n_scalars::Integer, capacity::Integer)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:bdf_diag_create, lib), Cint, (Ptr{Cvoid}, Int64, Cint, Int64, Ref{Ptr{Cvoid}}), c.h, n_cells, n_scalars, capacity, out))
        d = new(out[], c, n_cells, n_scalars)
        finalizer(x -> ccall((:bdf_diag_destroy, lib), Cint, (Ptr{Cvoid},), x.h), d)
        d
    end
end
"this draw's predictions (as predict! forms them), its sum of squared errors and its alpha (alpha_dev, a device Float64, wins) into the next row"
diag_push!(c::Context, d::Diag, p::DevPairs, D::Integer, factors::Vector{Ptr{Cvoid}}, mean_value, alpha::Real,
           alpha_dev::Union{DevArray{Float64},Nothing}=nothing) =
    check(ccall((:bdf_diag_push, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Float64, Ptr{Cvoid}),
                c.h, d.h, p.h, D, factors, mean_value, alpha, alpha_dev === nothing ? C_NULL : alpha_dev.p))
"parity hooks: row `draw` (0-based) of the plane from values (device, n_cells + n_scalars Float64); (the plane's device address, the draws it holds)"
diag_write!(d::Diag, draw::Integer, values::DevArray{Float64}) =
    check(ccall((:bdf_diag_write, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}), d.h, draw, values.p))
function diag_plane(d::Diag)
    p = Ref{Ptr{Cvoid}}(C_NULL); n = Ref{Int64}(0)
    check(ccall((:bdf_diag_plane, lib), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Int64}), d.h, p, n))
    p[], n[]
end
"split R-hat, effective sample size and Monte Carlo standard error per series: out (device, n_cells x 3, or C_NULL) at the caller's index
orig[storage position] (device Int32, or C_NULL); stats (device, 6 + 3 n_scalars): max R-hat, min ESS, the counts of R-hat > rhat_cut, of
ESS < ess_cut and of cells without figures, the draws, then the scalars' triples"
diag_compute!(c::Context, d::Diag, orig::Ptr{Cvoid}, rhat_cut::Real, ess_cut::Real, out::Ptr{Cvoid}, stats::DevArray{Float64}) =
    check(ccall((:bdf_diag_compute, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, d.h, orig, rhat_cut, ess_cut, out, stats.p))
"out = mean_value + F beta: linear_values (macau.jl:91) and the test rows' baseline"
feat_linear!(c::Context, f::Ptr{Cvoid}, beta::DevArray{Float64}, mean_value, out::DevArray{Float64}) =
    check(ccall((:bdf_feat_linear, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ptr{Cvoid}), c.h, f, beta.p, mean_value, out.p))
"store the pairs sorted by their id in `mode` (1-based): halves the gather traffic of the updates; results stay in the caller's order"
pairs_sort!(p::DevPairs, mode::Integer) = check(ccall((:bdf_pairs_sort, lib), Cint, (Ptr{Cvoid}, Cint), p.h, mode - 1))
"storage position -> the caller's index (1-based) after pairs_sort!"
function pairs_order(p::DevPairs)
    o = zeros(Int64, p.n)
    check(ccall((:bdf_pairs_order, lib), Cint, (Ptr{Cvoid}, Ptr{Int64}), p.h, o))
    return o .+ 1
end
"running posterior mean and sum of squares of the pairs (macau.jl:171-183, 235-241), in STORAGE order (pairs_order)"
function pairs_state(c::Context, p::DevPairs)
    a = Ref{Ptr{Cvoid}}(C_NULL); q = Ref{Ptr{Cvoid}}(C_NULL); n = Ref{Int64}(0)
    check(ccall((:bdf_pairs_state, lib), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Ptr{Cvoid}}, Ref{Int64}), p.h, a, q, n))
    avg = zeros(n[]); sq = zeros(n[])
    if n[] > 0
        check(ccall((:bdf_d2h, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), c.h, avg, a[], 8 * n[]))
        check(ccall((:bdf_d2h, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Csize_t), c.h, sq, q[], 8 * n[]))
    end
    return avg, sq
end
# ---- the ordinal noise model: sampled cutpoints (csrc/k_ordinal.hip) --------------------------------------------------------
"the edges of an ordinal relation with levels 1 .. K (4 <= K <= 16), their Metropolis step's size and counters, and a trace of
`trace_capacity` rows, on the device"
mutable struct Ordinal
    h::Ptr{Cvoid}
    ctx::Context
    K::Int
    capacity::Int
    function Ordinal(c::Context, K::Integer, step::Real=0.1, trace_capacity::Integer=0)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:bdf_ordinal_create, lib), Cint, (Ptr{Cvoid}, Cint, Float64, Int64, Ref{Ptr{Cvoid}}), c.h, K, step, trace_capacity, out))
        o = new(out[], c, K, trace_capacity)
        finalizer(x -> ccall((:bdf_ordinal_destroy, lib), Cint, (Ptr{Cvoid},), x.h), o)
        o
    end
end
"how many steps adapt the step size under adapt = -1 (the burn-in's length)"
ordinal_set_adapt!(o::Ordinal, steps::Integer) = check(ccall((:bdf_ordinal_set_adapt, lib), Cint, (Ptr{Cvoid}, Int64), o.h, steps))
"one Metropolis step on the edges with the latents integrated out, then the rows' bounds (device Float64, 2 x n, rewritten when the
proposal was accepted); `codes`: device Int8 levels of `train` in the caller's order; adapt: 1, 0 or -1 (by ordinal_set_adapt!)"
function ordinal_step!(c::Context, o::Ordinal, train::DevPairs, codes::DevArray{Int8}, D, factors::Vector{<:DevArray}, mean_value, alpha, alpha_dev,
                       rel_tag, adapt::Integer, bounds::DevArray{Float64})
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_ordinal_step, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Float64, Ptr{Cvoid}, UInt32, Cint, Ptr{Cvoid}),
                c.h, o.h, train.h, codes.p, D, fp, mean_value, alpha, alpha_dev === nothing ? C_NULL : alpha_dev.p, rel_tag, adapt, bounds.p))
end
"bounds (device Float64, 2 x n) of the levels in `codes` (device Int8, n) under the current edges: held-out cells' bins"
ordinal_bounds!(c::Context, o::Ordinal, codes::DevArray{Int8}, n::Integer, bounds::DevArray{Float64}) =
    check(ccall((:bdf_ordinal_bounds, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}), c.h, o.h, codes.p, n, bounds.p))
"(edges e_1 .. e_{K-1}, sigma, proposals, accepts, the last step's S, the first `rows` rows of the trace as a (K - 1) x rows matrix);
waits for the stream of the last step"
function ordinal_read(o::Ordinal, rows::Integer=0)
    edges, sigma, np, na, S = zeros(o.K - 1), Ref(0.0), Ref{Int64}(0), Ref{Int64}(0), Ref(0.0)
    trace = zeros(o.K - 1, rows)
    check(ccall((:bdf_ordinal_read, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}, Ref{Int64}, Ref{Int64}, Ref{Float64}, Ptr{Float64}, Int64),
                o.h, edges, sigma, np, na, S, trace, rows))
    return edges, sigma[], np[], na[], S[], trace
end
"(parity checks) the last step's proposed edges, its Jacobian term, whether it was accepted and the log of its uniform"
function ordinal_proposal(o::Ordinal)
    edges, jac, acc, lu = zeros(o.K - 1), Ref(0.0), Ref{Cint}(0), Ref(0.0)
    check(ccall((:bdf_ordinal_proposal, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ref{Float64}, Ref{Cint}, Ref{Float64}), o.h, edges, jac, acc, lu))
    return edges, jac[], acc[] != 0, lu[]
end

"one scoring step of the held-out log predictive density on the pairs: the log-likelihood l of every pair's kind of record given
the factors (probit link: log Phi(+-m); `bounds` -- device Float64, 2 x n, column k the (lower, upper) of pair k in the caller's
order, or `nothing` -- with lower < upper: the interval's mass; otherwise the Gaussian density at the stored value), folded into
the pairs' streaming log-sum-exp (phase 0 burn-in: nothing kept; 1 first posterior draw; 2 later ones); `alpha_dev` (a device
scalar or `nothing`) wins over `alpha`; stats (DevArray of 4 doubles): sum of l, sum of lpd, 0, 0"
function pairs_lpd_update!(c::Context, p::DevPairs, bounds, D, factors::Vector{<:DevArray}, mean_value, alpha, alpha_dev, phase::Integer,
                           stats::DevArray{Float64})
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_pairs_lpd_update, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Float64, Ptr{Cvoid}, Cint, Ptr{Cvoid}),
                c.h, p.h, bounds === nothing ? C_NULL : bounds.p, D, fp, mean_value, alpha, alpha_dev === nothing ? C_NULL : alpha_dev.p,
                phase, stats.p))
end
"lpd of every pair over the posterior draws scored so far -> out (DevArray of n doubles), in the caller's order"
pairs_lpd!(c::Context, p::DevPairs, out::DevArray{Float64}) =
    check(ccall((:bdf_pairs_lpd, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), c.h, p.h, out.p))

"one scoring step of WAIC on the pairs (the training table): the log-likelihood l of `pairs_lpd_update!` -- the same arguments and
phases, but with `bounds` the pairs' baseline is not read -- folded into the pairs' streaming log-sum-exp and Welford's mean and M2
of l; stats (DevArray of 4 doubles): sum of l, sum of lppd, sum of V (the variance of l over the draws), the count of V > 0.4"
function pairs_waic_update!(c::Context, p::DevPairs, bounds, D, factors::Vector{<:DevArray}, mean_value, alpha, alpha_dev, phase::Integer,
                            stats::DevArray{Float64})
    fp = Ptr{Cvoid}[f.p for f in factors]
    check(ccall((:bdf_pairs_waic_update, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Ptr{Cvoid}}, Float64, Float64, Ptr{Cvoid}, Cint, Ptr{Cvoid}),
                c.h, p.h, bounds === nothing ? C_NULL : bounds.p, D, fp, mean_value, alpha, alpha_dev === nothing ? C_NULL : alpha_dev.p,
                phase, stats.p))
end
"the end of the run: (lppd, V) of every pair -> out (DevArray of 2 x n doubles in the caller's order, or `nothing`); stats (DevArray
of 4 doubles): sum of lppd, sum of V, sum of (elpd - mean elpd)^2, the count of V > 0.4"
pairs_waic!(c::Context, p::DevPairs, out, stats::DevArray{Float64}) =
    check(ccall((:bdf_pairs_waic, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), c.h, p.h, out === nothing ? C_NULL : out.p, stats.p))

# ---- cells of rows that were not in training (setNewRows / setNewTest) ------------------------------------------------------
"q[j] = v_j' Lambda^-1 v_j for the M rows of V (DevArray D x M): the variance that a new row's own factor, u* ~ N(uhat, Lambda^-1), adds
to a cell of column j; Lambda = L L' is factorised once per call and q = |L^-1 v|^2 is formed on the matrix cores"
newrows_quad!(c::Context, D, M, Lambda::DevArray{Float64}, V::DevArray{Float64}, q::DevArray{Float64}) =
    check(ccall((:bdf_newrows_quad, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), c.h, D, M, Lambda.p, V.p, q.p))
"one prediction step on the new cells `p` (first-mode ids index the columns of `uhat_new`, D x n*; second-mode ids those of V and q):
the new row's factor integrated out in closed form, folded into the pairs' running state (phase 0 burn-in: nothing kept; 1 first
posterior draw; 2 later ones); stats (DevArray of 8 doubles): SSE of the running mean, SSE of this draw, the two correct-counts at
class_cut, the count of cells with a value, sum of lpd, sum of this draw's log-likelihoods, 0"
function newrows_update!(c::Context, p::DevPairs, D, uhat_new::DevArray{Float64}, V::DevArray{Float64}, q::DevArray{Float64}, mean_value,
                         alpha, alpha_dev, phase::Integer, clamp_lo, clamp_hi, class_cut, score_lpd::Bool, stats::DevArray{Float64})
    check(ccall((:bdf_newrows_update, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64, Ptr{Cvoid}, Cint, Float64, Float64, Float64, Cint,
                 Ptr{Cvoid}),
                c.h, p.h, D, uhat_new.p, V.p, q.p, mean_value, alpha, alpha_dev === nothing ? C_NULL : alpha_dev.p, phase, clamp_lo, clamp_hi,
                class_cut, score_lpd ? 1 : 0, stats.p))
end
"(pred, stdev, lpd) of every new cell -> out (DevArray of 3 x n doubles), in the caller's order"
newrows_result!(c::Context, p::DevPairs, out::DevArray{Float64}) =
    check(ccall((:bdf_newrows_result, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), c.h, p.h, out.p))
# ---- new rows conditioned on a few cells of their own: the fold-in (setNewObserved) ------------------------------------------------
"one draw's fold-in: `known` is ONE term of the two-mode relation of the known cells (n_new x M, mode 0) whose other-mode factor is this
draw's V and whose alpha is the draw's; per new row P_i = Lambda + alpha sum v v', uhat_i = P_i^-1 b_i by the row sampler's own
accumulation and a workgroup of four waves per row (one factorises, all four share the row's cells), and per cell of `cells` (stored sorted by the new row) m = mean_value + uhat_i . v_j
and q = v_j' P_i^-1 v_j into m, q (DevArrays of n doubles, storage order); uhat (DevArray D x n_new) for every new row"
function foldin_cells!(c::Context, D, n_new, known::Term, mu::DevArray{Float64}, mu_is_matrix::Bool, Lambda::DevArray{Float64}, cells::DevPairs,
                       mean_value, m::DevArray{Float64}, q::DevArray{Float64}, uhat::DevArray{Float64})
    check(ccall((:bdf_foldin_cells, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ref{Term}, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, D, n_new, Ref(known), mu.p, mu_is_matrix ? 1 : 0, Lambda.p, cells.h, mean_value, m.p, q.p, uhat.p))
end
"(parity hook) the fold-in's second half on given systems in row_system's layout: P (D x D x n_new), b (D x n_new), V (D x M)"
function foldin_solve!(c::Context, D, n_new, P::DevArray{Float64}, b::DevArray{Float64}, cells::DevPairs, M, V::DevArray{Float64}, mean_value,
                       m::DevArray{Float64}, q::DevArray{Float64}, uhat::DevArray{Float64})
    check(ccall((:bdf_foldin_solve, lib), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Float64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, D, n_new, P.p, b.p, cells.h, M, V.p, mean_value, m.p, q.p, uhat.p))
end
"newrows_update! on (m, q) per cell (DevArrays of n doubles in the pairs' storage order: foldin_cells!'s output) instead of the gather:
the same link, fold, phases, stats and running state"
function newrows_update_cells!(c::Context, p::DevPairs, m::DevArray{Float64}, q::DevArray{Float64}, alpha, alpha_dev, phase::Integer, clamp_lo,
                               clamp_hi, class_cut, score_lpd::Bool, stats::DevArray{Float64})
    check(ccall((:bdf_newrows_update_cells, lib), Cint,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ptr{Cvoid}, Cint, Float64, Float64, Float64, Cint, Ptr{Cvoid}),
                c.h, p.h, m.p, q.p, alpha, alpha_dev === nothing ? C_NULL : alpha_dev.p, phase, clamp_lo, clamp_hi, class_cut, score_lpd ? 1 : 0,
                stats.p))
end
"(parity hook) the device address of the new cells' running state (five planes of n doubles in storage order) and its draw count"
function newrows_state(p::DevPairs)
    st, draws = Ref{Ptr{Cvoid}}(C_NULL), Ref(0.0)
    check(ccall((:bdf_newrows_state, lib), Cint, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}, Ref{Float64}), p.h, st, draws))
    return st[], draws[]
end

# ---- AUC_ROC (src/ROC.jl:1-11) and vecnorm on the device ------------------------------------------------------------------
"AUC_ROC(Ytrue, scores) of device arrays (labels: UInt8, nonzero = positive): (auc, C, P, Nn), C the exact pair count"
function auc_roc(c::Context, labels::DevArray{UInt8}, scores::DevArray{Float64})
    n = prod(scores.dims)
    ws = DevArray(c, zeros(UInt8, max(ccall((:bdf_auc_workspace_bytes, lib), Int64, (Int64,), n), 1)))
    out, counts = DevArray(c, zeros(1)), DevArray(c, zeros(Int64, 3))
    check(ccall((:bdf_auc_roc, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, n, labels.p, scores.p, ws.p, out.p, counts.p))
    k = Array(counts)
    (Array(out)[1], k[1], k[2], k[3])
end
"roc_avg of macau.jl:200, AUC_ROC(values .< class_cut, -avg), over the pairs' running mean -> out (DevArray of 1 double);
 `c` is the context whose stream ran the prediction update"
pairs_auc!(c::Context, p::DevPairs, class_cut, out::DevArray{Float64}) =
    check(ccall((:bdf_pairs_auc, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Ptr{Cvoid}, Ptr{Cvoid}), c.h, p.h, class_cut, out.p, C_NULL))
"vecnorm(x) of a device array, summed in a fixed order -> out (DevArray of 1 double)"
norm2!(c::Context, x::DevArray{Float64}, out::DevArray{Float64}) =
    check(ccall((:bdf_norm2, lib), Cint, (Ptr{Cvoid}, Int64, Ptr{Cvoid}, Ptr{Cvoid}), c.h, prod(x.dims), x.p, out.p))

# ---- feature operators on several ranks; the hyperprior's sums over the ranks ----------------------------------------------
"original id (0-based) of every row of F: rows moved to an entity's internal positions keep their noise streams (several GPUs)"
feat_set_row_ids!(f::Ptr{Cvoid}, row_ids::Vector{Int32}) = check(ccall((:bdf_feat_set_row_ids, lib), Cint, (Ptr{Cvoid}, Ptr{Int32}), f, row_ids))
function feat_size(f::Ptr{Cvoid})
    m = Ref{Int64}(0); n = Ref{Int64}(0); z = Ref{Int64}(0)
    check(ccall((:bdf_feat_size, lib), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}), f, m, n, z))
    return m[], n[], z[]
end
"sum_i U_i and U U' over the rows this rank owns, the ranks' partial sums added in rank order (src/sampling.jl:117-119 on the master)"
hyper_sums!(c::Context, m::Comm, D, N, chunks, sample::DevArray, uhat, sumU::DevArray, UUt::DevArray) =
    check(ccall((:bdf_hyper_sums_ranks, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Int64, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                c.h, m.h, D, N, chunks, sample.p, uhat === nothing ? C_NULL : uhat.p, sumU.p, UUt.p))
"the data-independent part of the hyperprior draw (Bartlett matrix, mean normals), ahead of the rows: D*D + D doubles"
hyper_draws!(c::Context, D, N, nu, entity_tag, draws::DevArray{Float64}) =
    check(ccall((:bdf_hyper_draws, lib), Cint, (Ptr{Cvoid}, Cint, Int64, Float64, UInt32, Ptr{Cvoid}), c.h, D, N, nu, entity_tag, draws.p))
prior_pack_doubles(D::Integer) = Int(ccall((:bdf_prior_pack_doubles, lib), Cint, (Cint,), D))

# ---- the relation model inside the native iteration (src/macau.jl:83-92; bdf_gibbs_set_relations) ----------------------------
struct GibbsRelation                              # bdf_gibbs_relation, field for field
    rel::Ptr{Cvoid}
    entity_of_mode::NTuple{4,Int32}
    mean_value::Float64
    alpha_dev::Ptr{Cvoid}
    alpha_sample::Int32
    rel_tag::UInt32
    alpha_lambda0::Float64
    alpha_nu0::Float64
    nnz::Int64
    train::Ptr{Cvoid}
    first_obs::Int64
    obs_block::Int64
    feat::Ptr{Cvoid}
    beta::Ptr{Cvoid}
    linear::Ptr{Cvoid}
    lambda_beta::Float64
    feat_test::Ptr{Cvoid}
    test_baseline::Ptr{Cvoid}
    probit::Int32                                 # probit noise model: the latent draw before the rows (needs train and linear)
    _pad::Int32
    censor::Ptr{Cvoid}                            # censored noise model: device Int8 flags per observation of train (C_NULL: none)
    interval::Ptr{Cvoid}                          # interval-censored noise model: device Float64 (lower, upper) per observation of train (C_NULL: none)
    ordinal::Ptr{Cvoid}                           # ordinal noise model: an Ordinal's handle (C_NULL: none); needs interval
    ordinal_codes::Ptr{Cvoid}                     # ... and device Int8 levels 1 .. K per observation of train
    robust_nu::Float64                            # robust (Student-t) noise model: its degrees of freedom >= 1 (0: off)
    obs_precision::Ptr{Cvoid}                     # device Float64 weight per observation of train: robust_draw!'s omega, or the caller's (C_NULL: none)
    pg_model::Int32                               # Polya-Gamma noise model: 1 logit, 2 counts (0: none); pg_draw! rewrites obs_precision and linear
    _pad_pg::Int32
    pg_r::Float64                                 # ... the counts' integer dispersion r >= 1
    bg_weight::Float64                            # background cells: every unlisted cell observes bg_value with precision alpha bg_weight (0: none)
    bg_value::Float64
    bg_sums::Ptr{Cvoid}                           # device, 2 (D + D D) Float64: per mode, the sum of its rows and their Gram matrix
    bg_weights::Ptr{Cvoid}                        # device Float64 omega_k per observation of train (C_NULL: 1); obs_precision then holds omega_k - bg_weight
    noise_mode::Int32                             # a noise precision per row of the entity at this 1-based mode (0: none); entity_noise_draw! rewrites noise_tau and obs_precision
    _pad_noise::Int32
    noise_shape::Float64                          # ... tau_j ~ Gamma(noise_shape, noise_rate) a priori
    noise_rate::Float64
    noise_tau::Ptr{Cvoid}                         # device Float64 per row of that mode: the last draw
    dense_R::Ptr{Cvoid}                           # a dense relation (C_NULL: none): device N x M Float64 row-major, every cell without its mean; rel then lists no cell
    dense_C::Ptr{Cvoid}                           # device (N + M) x D Float64: the rows of R V for mode 1, then of R' U for mode 2 (dense_product!)
    dense_sums::Ptr{Cvoid}                        # device, 2 (D + D D) Float64: as bg_sums
    dense_sum_r2::Float64                         # the listed cells' sum of r^2
    dense_holes::Ptr{Cvoid}                       # bdf_pairs of the cells that are not listed (C_NULL: none): dense_impute! draws them before every iteration
    dense_stats::Ptr{Cvoid}                       # device, 4 Float64 (C_NULL without holes): [1] the holes' sum of r^2
    n_bias::Int32                                 # row and column biases: the number of biased modes (0: none); bias_draw! rewrites the terms' bias and lambda, and linear
    _pad_bias::Int32
    bias::NTuple{4,BiasTerm}                      # ... the first n_bias are read
    bias_resid::Ptr{Cvoid}                        # ... device Float64 per observation of train (scratch)
    bias_test::Ptr{Cvoid}                         # ... bdf_pairs whose baseline test_baseline is refreshed after the draw (C_NULL: none)
end
"register the relations whose alpha is sampled and / or that carry features: sweep! then runs sample_alpha, sample_beta_rel and
linear_values before the rows of every iteration; `keep`: what the records point into"
function set_relations!(g::Gibbs, rels::Vector{GibbsRelation}; keep::Vector=Any[])
    check(ccall((:bdf_gibbs_set_relations, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{GibbsRelation}), g.h, length(rels), rels))
    append!(g.keep, keep)
    nothing
end

# ---- variational BPMF (src/macau_vb.jl; bdf_vb_*) --------------------------------------------------------------------------
"The device side of bpmf_vb: both entities' VB models of relations[1] (bdf_vb_create, macau_vb.jl:20-58)."
mutable struct VB
    h::Ptr{Cvoid}
    ctx::Context
    D::Int
    N::Tuple{Int,Int}
    test::Any                         # the test pairs it borrows
    function VB(c::Context, D::Integer, ids::Matrix{Int64}, values::Vector{Float64}, dims::Vector{Int64}, alpha::Float64,
                mu_u::Matrix{Float64}, mu_v::Matrix{Float64})
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:bdf_vb_create, lib), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Ptr{Cvoid}, Cint, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ref{Ptr{Cvoid}}),
                    c.h, D, dims, size(ids, 1), ids, 8, values, alpha, mu_u, mu_v, out))
        v = new(out[], c, Int(D), (Int(dims[1]), Int(dims[2])), nothing)
        finalizer(x -> ccall((:bdf_vb_destroy, lib), Cint, (Ptr{Cvoid},), x.h), v)
        v
    end
end
"test_vec (macau_vb.jl:56-58) as DevPairs (C_NULL: none; `keep` holds them) and the clamp of clamp! (src/sampling.jl:108-114)"
function vb_set_test!(v::VB, pairs::Ptr{Cvoid}, clamp::Vector{Float64}; keep=nothing)
    lo, hi = isempty(clamp) ? (1.0, 0.0) : (clamp[1], clamp[2])
    v.test = keep
    check(ccall((:bdf_vb_set_test, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64), v.h, pairs, lo, hi))
end
"n iterations of macau_vb.jl:61-77 (update_u! twice, update_prior! twice, the two RMSEs), enqueued without a host round trip"
vb_iterate!(v::VB, n::Integer) = check(ccall((:bdf_vb_iterate, lib), Cint, (Ptr{Cvoid}, Cint), v.h, n))
"(rmse, rmse_train, vecnorm(U.mu_u), vecnorm(V.mu_u)) of the last iteration (macau_vb.jl:80); waits for the device"
function vb_stats(v::VB)
    out = zeros(4)
    check(ccall((:bdf_vb_stats, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}), v.h, out))
    (out[1], out[2], out[3], out[4])
end
"host copy of entity e's model (1 = U, 2 = V): mu_u (D x N), Euu (D x D x N), mu_N, W_N, nu_N, b_N"
function vb_model(v::VB, e::Integer)
    D, N = v.D, v.N[e]
    mu, Euu, prior = zeros(D, N), zeros(D, D, N), zeros(D + D * D + 2)
    check(ccall((:bdf_vb_model, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}), v.h, e - 1, mu, Euu, prior))
    (mu, Euu, prior[1:D], reshape(prior[D+1:D+D*D], D, D), prior[D+D*D+1], prior[D+D*D+2])
end

"""
    bpmf_vb(data; num_latent=10, verbose=true, niter=100, clamp=Float64[])

Replaces `bpmf_vb` (src/macau_vb.jl:39-90): the same set-up (VBModel draws its means with randn, U first), the iterations on
the device, and the reference's Dict of host VBModels.  The VBModel type is the reference's.
"""
function bpmf_vb(data; num_latent::Int=10, verbose::Bool=true, niter::Int=100, clamp::Vector{Float64}=Float64[], device::Integer=0)
    rel = data.relations[1]
    size(rel.data.df, 2) == 3 || throw(ArgumentError("bpmf_vb works on a matrix relation (2 modes)"))
    1 <= num_latent <= 64 || throw(ArgumentError("num_latent must be in 1..64"))
    Umodel = Main.BayesianDataFusion.VBModel(num_latent, data.entities[1].count)
    Vmodel = Main.BayesianDataFusion.VBModel(num_latent, data.entities[2].count)
    alpha = rel.model.alpha
    result = Dict("Umodel" => Umodel, "Vmodel" => Vmodel, "rmse" => NaN, "rmse_train" => NaN, "alpha" => alpha)
    niter > 0 || return result
    df = rel.data.df
    ids = hcat(convert(Vector{Int64}, df[:, 1]), convert(Vector{Int64}, df[:, 2]))
    c = Context(device)
    v = VB(c, num_latent, ids, convert(Vector{Float64}, df[:, 3]), Int64[size(Umodel.mu_u, 2), size(Vmodel.mu_u, 2)],
           alpha, Umodel.mu_u, Vmodel.mu_u)
    tv = rel.test_vec
    if size(tv, 1) > 0
        tids = hcat(convert(Vector{Int64}, tv[:, 1]), convert(Vector{Int64}, tv[:, 2]))
        test = DevPairs(c, tids, convert(Vector{Float64}, tv[:, 3]))
        vb_set_test!(v, test.h, clamp; keep=test)
    else
        vb_set_test!(v, C_NULL, clamp)
    end
    st = (NaN, NaN, 0.0, 0.0)
    for i in 1:(verbose ? niter : 1)
        time0 = time()
        vb_iterate!(v, verbose ? 1 : niter)
        st = vb_stats(v)
        verbose && @printf("% 3d: |U|=%.4e  |V|=%.4e  RMSE=%.4f  RMSE(train)=%.4f  [took %.2fs]\n", i, st[3], st[4], st[1], st[2], time() - time0)
    end
    for (e, m) in ((1, Umodel), (2, Vmodel))
        m.mu_u, m.Euu, m.mu_N, m.W_N, m.nu_N, m.b_N = vb_model(v, e)
    end
    result["rmse"], result["rmse_train"] = st[1], st[2]
    result
end


# ---- Hamiltonian Monte Carlo BPMF (src/macau_hmc.jl; bdf_hmc_*) -------------------------------------------------------------
"The device side of macau_hmc: both entities' samples, momenta and priors of relations[1] after reset! (bdf_hmc_create)."
mutable struct HMC
    h::Ptr{Cvoid}
    ctx::Context
    D::Int
    N::Tuple{Int,Int}
    test::Any                         # the test pairs it borrows
    function HMC(c::Context, D::Integer, ids::Matrix{Int64}, values::Vector{Float64}, dims::Vector{Int64}, alpha::Float64)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:bdf_hmc_create, lib), Cint,
                    (Ptr{Cvoid}, Cint, Ptr{Int64}, Int64, Ptr{Cvoid}, Cint, Ptr{Float64}, Float64, Ref{Ptr{Cvoid}}),
                    c.h, D, dims, size(ids, 1), ids, 8, values, alpha, out))
        v = new(out[], c, Int(D), (Int(dims[1]), Int(dims[2])), nothing)
        finalizer(x -> ccall((:bdf_hmc_destroy, lib), Cint, (Ptr{Cvoid},), x.h), v)
        v
    end
end
"test_vec (macau_hmc.jl:48-52) as DevPairs (C_NULL: none; `keep` holds them) and the clamp of clamp! (src/sampling.jl:108-114)"
function hmc_set_test!(v::HMC, pairs::Ptr{Cvoid}, clamp::Vector{Float64}; keep=nothing)
    lo, hi = isempty(clamp) ? (1.0, 0.0) : (clamp[1], clamp[2])
    v.test = keep
    check(ccall((:bdf_hmc_set_test, lib), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Float64, Float64), v.h, pairs, lo, hi))
end
"macau_hmc's keyword arguments L, L_inner, prior_freq, eps, burnin (eps and L then adapt)"
hmc_set_params!(v::HMC, L::Integer, L_inner::Integer, prior_freq::Integer, eps::Float64, burnin::Integer) =
    check(ccall((:bdf_hmc_set_params, lib), Cint, (Ptr{Cvoid}, Cint, Cint, Cint, Float64, Cint), v.h, L, L_inner, prior_freq, eps, burnin))
"n iterations of macau_hmc.jl:60-132 (one small device-to-host read per iteration for the adapted L)"
hmc_iterate!(v::HMC, n::Integer) = check(ccall((:bdf_hmc_iterate, lib), Cint, (Ptr{Cvoid}, Cint), v.h, n))
"the last iteration's record (16 doubles, include/bdf.h) and its momentum-norm log (2L + 1 values); waits for the device"
function hmc_stats(v::HMC)
    out = zeros(16)
    check(ccall((:bdf_hmc_stats, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint), v.h, out, C_NULL, 0))
    log = zeros(2 * Int(out[3]) + 1)
    check(ccall((:bdf_hmc_stats, lib), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Cint), v.h, out, log, length(log)))
    (out, log)
end
"host copy of entity e (1 = U, 2 = V): sample (D x N), momentum (D x N), mu, Lambda"
function hmc_model(v::HMC, e::Integer)
    D, N = v.D, v.N[e]
    sample, momentum, mu, Lambda = zeros(D, N), zeros(D, N), zeros(D), zeros(D, D)
    check(ccall((:bdf_hmc_model, lib), Cint, (Ptr{Cvoid}, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                v.h, e - 1, sample, momentum, mu, Lambda))
    (sample, momentum, mu, Lambda)
end

"""
    macau_hmc(data; num_latent=10, verbose=true, burnin=100, psamples=100, L=10, L_inner=1, prior_freq=8, eps=0.01,
              reset_model=true, clamp=Float64[])

Replaces `macau_hmc` (src/macau_hmc.jl:20-137): the iterations on the device (from reset!), the reference's verbose lines,
the entities' samples, mu and Lambda written back, and the reference's Dict.
"""
function macau_hmc(data; num_latent::Int=10, verbose::Bool=true, burnin::Int=100, psamples::Int=100, L::Int=10, L_inner::Int=1,
                   prior_freq::Int=8, eps::Float64=0.01, reset_model=true, clamp::Vector{Float64}=Float64[], device::Integer=0)
    rel = data.relations[1]
    size(rel.data.df, 2) == 3 || throw(ArgumentError("macau_hmc works on a matrix relation (2 modes)"))
    1 <= num_latent <= 64 || throw(ArgumentError("num_latent must be in 1..64"))
    reset_model || throw(ArgumentError("macau_hmc starts from reset!: reset_model=false is not supported"))
    verbose && println("Model setup")
    df = rel.data.df
    ids = hcat(convert(Vector{Int64}, df[:, 1]), convert(Vector{Int64}, df[:, 2]))
    alpha = rel.model.alpha
    c = Context(device)
    v = HMC(c, num_latent, ids, convert(Vector{Float64}, df[:, 3]), Int64[data.entities[1].count, data.entities[2].count], alpha)
    tv = rel.test_vec
    if size(tv, 1) > 0
        tids = hcat(convert(Vector{Int64}, tv[:, 1]), convert(Vector{Int64}, tv[:, 2]))
        test = DevPairs(c, tids, convert(Vector{Float64}, tv[:, 3]))
        hmc_set_test!(v, test.h, clamp; keep=test)
    else
        hmc_set_test!(v, C_NULL, clamp)
    end
    hmc_set_params!(v, L, L_inner, prior_freq, eps, burnin)
    st = fill(NaN, 16)
    for i in 1:(burnin + psamples)
        time0 = time()
        hmc_iterate!(v, 1)
        st, lg = hmc_stats(v)
        if verbose
            Lu = Int(st[3])
            i == burnin + 1 && print("================== Burnin complete ===================\n")
            @printf("======= Step %d =======\n", i)
            @printf("eps = %.2e\n", st[2])
            for l in 1:Lu
                @printf("  Momentum %d: |r_U| = %.4e, |r_V| = %.4e\n", l, lg[l < Lu ? 2l + 1 : 2l - 1], lg[2l])
            end
            @printf("  Momentum L: |r_U| = %.4e, |r_V| = %.4e\n", lg[2Lu + 1], lg[2Lu])
            @printf("  ΔH = %.4e  ΔKin = %.4e  ΔPot = %.4e\n", -st[8], st[5] - st[4], st[7] - st[6])
            if st[9] != 0
                print("-> ACCEPTED!\n")
            else
                print("-> REJECTED!\n")
                if st[8] < -6
                    @printf("Reducing eps from %.2e to %.2e.\n", st[2], st[10])
                    @printf("Increasing L from %d to %d.\n", Lu, Int(st[11]))
                end
            end
            i % prior_freq == 0 && println("Updating priors...")
            @printf("% 3d: |U|=%.4e  |V|=%.4e  RMSE=%.4f  RMSE(avg)=%.4f [took %.2fs]\n", i, st[12], st[13], st[15], st[16], time() - time0)
        end
    end
    for e in 1:2
        m = data.entities[e].model
        m.sample, _, m.mu, m.Lambda = hmc_model(v, e)
    end
    Dict("rmse" => st[15], "rmse_train" => NaN, "alpha" => alpha)
end

end # module
