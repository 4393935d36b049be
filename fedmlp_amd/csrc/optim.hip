// Optimizer kernels over the engine's flat arenas (weights, gradient, moments: NP floats each, NP a multiple of 4): torch.optim
// Adam (coupled L2: the fused steps' optimizer and fm_adam_step's), AdamW and SGD, each in a flat form over the whole arena and
// in a form over the entry table for parameter groups and frozen entries; the gradient accumulator's passes, the L2 norm of the
// accumulator and the two clips.  gfx950.
//
// All of them stream the arena once in 16-byte elements on the main lane's stream, take the engine's skip word (a kernel of
// this step reported a lost part -- pconv.hip's bounded stream-K wait -- so the gradients are poisoned: nothing is written, and
// the host learns of it through the word's mapped twin at its next call) and never synchronise with the host.  The flat
// element-wise ones run one 16-byte element per thread (k_bn_bwd_apply's launcher has the measurement).
// Bytes moved per parameter: SGD 12 (no momentum) / 20, Adam and AdamW 28, accumulate 8 / 12, norm 4, clip 8.
#include "common.h"
#include "kernels.h"

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ------------------------------------------------------- the update rules --------
// Each rule is stated ONCE: update(Quad&, Hp) holds its arithmetic for the four floats of a 16-byte element, and both the flat
// kernels and the parameter-group kernels below call it, so the two forms compute the same bits by construction
// (tests/test_param_groups_gpu.py compares them).  Every update is written under `fp contract(off)` with each multiply-add an
// explicit fma: which product joins which addition decides the last bit, and left to the compiler that choice is made per
// inlining -- it differed between two kernels holding the same AdamW expressions.  The fmas spelled out are the ones the
// kernels held when each rule was still written as plain expressions, so the trajectories recorded then still hold.
// A rule also carries its operand arenas: load() reads a quad of every operand at float offset o (a multiple of 4), store()
// writes the floats of the quad that lie in [begin, end) (arena_table.h: store_own, and the walker's concept).

// the operands of the two rules with two moments
struct PgmvRule {
    float* p; const float* g; float* m; float* v;
    struct Quad { f32x4 p, g, m, v; };
    __device__ __forceinline__ void load(Quad& q, int64_t o) const
    {
        q.p = *reinterpret_cast<const f32x4*>(p + o); q.g = *reinterpret_cast<const f32x4*>(g + o);
        q.m = *reinterpret_cast<const f32x4*>(m + o); q.v = *reinterpret_cast<const f32x4*>(v + o);
    }
    __device__ __forceinline__ void store(const Quad& q, int64_t o, int64_t begin, int64_t end) const
    {
        store_own(p, o, begin, end, q.p); store_own(m, o, begin, end, q.m); store_own(v, o, begin, end, q.v);
    }
};

// torch.optim.Adam's single-tensor update in its order, L2 decay folded into g: g += wd p; exp_avg.lerp_(g, 1 - beta1);
// exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) g g; denom = sqrt(exp_avg_sq) / sqrt(bc2) + eps; p -= lr / bc1 * exp_avg / denom.
// All in fp32 (the fused steps' golden trajectories are recorded with this lerp).
struct AdamRule : PgmvRule {
    using Hp = OptAdamHp;
    static __device__ __forceinline__ void update(Quad& q, const Hp& hp)
    {
#pragma clang fp contract(off)
        const float nstep = -(hp.lr / hp.bc1), one_minus_b1 = 1.f - hp.b1, one_minus_b2 = 1.f - hp.b2;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float g = __builtin_fmaf(hp.wd, q.p[k], q.g[k]);
            q.m[k] = __builtin_fmaf(one_minus_b1, g - q.m[k], q.m[k]);
            q.v[k] = __builtin_fmaf(q.v[k], hp.b2, (one_minus_b2 * g) * g);
            const float den = sqrtf(q.v[k]) / hp.bc2_sqrt + hp.eps;
            q.p[k] = __builtin_fmaf(nstep, q.m[k] / den, q.p[k]);
        }
    }
};

// torch.optim.AdamW's single-tensor update in its order: p *= 1 - lr wd; exp_avg.lerp_(g, 1 - beta1); exp_avg_sq = beta2
// exp_avg_sq + (1 - beta2) g g; denom = sqrt(exp_avg_sq) / sqrt(bc2) + eps; p -= lr / bc1 * exp_avg / denom.  No L2 in g.
// decay = 1 - lr wd and step = lr / bc1 are formed on the host in double.
struct AdamWRule : PgmvRule {
    using Hp = OptAdamWHp;
    static __device__ __forceinline__ void update(Quad& q, const Hp& hp)
    {
#pragma clang fp contract(off)
        const float one_minus_b2 = 1.f - hp.b2, nstep = -hp.step;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            q.v[k] = __builtin_fmaf(q.g[k], one_minus_b2 * q.g[k], q.v[k] * hp.b2);
            // the lerp in double, rounded once: where beta1 m and (1 - beta1) g cancel, an fp32 lerp is half an ulp of its OPERANDS
            // off, and lr / bc1 times that over denom is many ulps of a small p (SgdRule's note); everything after it carries
            // errors relative to the update itself and stays in fp32
            q.m[k] = (float)__builtin_fma(hp.one_minus_b1, (double)q.g[k] - (double)q.m[k], (double)q.m[k]);
            const float den = sqrtf(q.v[k]) / hp.bc2_sqrt + hp.eps;
            q.p[k] = __builtin_fmaf(hp.decay, q.p[k], nstep * (q.m[k] / den));       // (-step) x = -(step x), signed zeros included
        }
    }
};

// torch.optim.SGD's single-tensor update in its order: g += wd p; buf = g (first step after a reset) or momentum buf +
// (1 - dampening) g; g = nesterov ? g + momentum buf : buf; p -= lr g.
// MODE 0: momentum = 0, the buffer is neither read nor written; 1: first step (buf = g, no dampening: torch clones the
// gradient); 2: every later step.  A template argument, chosen by the launcher (flat) or by the block from its group's mode: one
// instantiation of the whole loop per MODE keeps the three expression trees apart (a run-time MODE inside the loop lets the
// compiler merge them).
// The chain is evaluated in double from the fp32 operands and each stored value (buf, p) is rounded once.  In fp32 the new p
// would inherit the rounding of momentum buf + (1 - dampening) g, half an ulp of its OPERANDS: where the two terms cancel and p is
// small against lr buf that is many ulps of p (tests/test_optim_gpu.py's bound, 4 ulp(p) + 1e-5 |dp|, is missed by a pure fp32
// chain, torch's own included).  Five double operations per parameter beside 12 / 20 bytes of HBM traffic: still a streaming kernel.
template <int MODE>
struct SgdRule {
    float* p; const float* g; float* buf;
    using Hp = OptSgdHp;
    struct Quad { f32x4 p, g, b; };
    __device__ __forceinline__ void load(Quad& q, int64_t o) const
    {
        q.p = *reinterpret_cast<const f32x4*>(p + o); q.g = *reinterpret_cast<const f32x4*>(g + o);
        q.b = f32x4{0.f, 0.f, 0.f, 0.f};
        if (MODE == 2) q.b = *reinterpret_cast<const f32x4*>(buf + o);
    }
    static __device__ __forceinline__ void update(Quad& q, const Hp& hp)
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double p = (double)q.p[k];
            double d = __builtin_fma(hp.wd, p, (double)q.g[k]);
            if (MODE != 0) {
                const double b = MODE == 1 ? d : __builtin_fma(hp.momentum, (double)q.b[k], hp.one_minus_damp * d);
                q.b[k] = (float)b;
                d = hp.nesterov ? __builtin_fma(hp.momentum, b, d) : b;
            }
            q.p[k] = (float)__builtin_fma(-hp.lr, d, p);
        }
    }
    __device__ __forceinline__ void store(const Quad& q, int64_t o, int64_t begin, int64_t end) const
    {
        if (MODE != 0) store_own(buf, o, begin, end, q.b);
        store_own(p, o, begin, end, q.p);
    }
};

// ------------------------------------------------------- the flat steps --------
// One quad per thread over the first n4 quads of the arenas; the quad is its own span, so store() is three (two, one) 16-byte
// stores.  adam_kernel is the same body under the name the fused steps' traces carry (tools/, profiles/).
template <class R>
__device__ __forceinline__ void opt_flat(const R& r, int64_t n4, const typename R::Hp& hp, const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    typename R::Quad q;
    r.load(q, 4 * i);
    R::update(q, hp);
    r.store(q, 4 * i, 4 * i, 4 * i + 4);
}
template <class R>
__global__ void opt_flat_kernel(const R r, int64_t n4, const typename R::Hp hp, const int* __restrict__ skip) { opt_flat(r, n4, hp, skip); }
__global__ void adam_kernel(const AdamRule r, int64_t n4, const OptAdamHp hp, const int* __restrict__ skip) { opt_flat(r, n4, hp, skip); }

void k_adam(float* p, const float* g, float* m, float* v, int64_t n, const OptAdamHp& hp, hipStream_t s, const int* skip)
{
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(adam_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, s, AdamRule{{p, g, m, v}}, n4, hp, skip);
}
void k_adamw(float* p, const float* g, float* m, float* v, int64_t n, const OptAdamWHp& hp, hipStream_t s, const int* skip)
{
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(opt_flat_kernel<AdamWRule>, dim3(cdiv(n4, 256)), dim3(256), 0, s, AdamWRule{{p, g, m, v}}, n4, hp, skip);
}
void k_sgd(float* p, const float* g, float* buf, int64_t n, const OptSgdHp& hp, hipStream_t s, const int* skip)
{
    const int64_t n4 = n / 4;
    const dim3 grid(cdiv(n4, 256)), block(256);
    if (hp.mode == 0) hipLaunchKernelGGL(opt_flat_kernel<SgdRule<0>>, grid, block, 0, s, SgdRule<0>{p, g, buf}, n4, hp, skip);
    else if (hp.mode == 1) hipLaunchKernelGGL(opt_flat_kernel<SgdRule<1>>, grid, block, 0, s, SgdRule<1>{p, g, buf}, n4, hp, skip);
    else hipLaunchKernelGGL(opt_flat_kernel<SgdRule<2>>, grid, block, 0, s, SgdRule<2>{p, g, buf}, n4, hp, skip);
}

// ------------------------------------------------------------- L2 norm ---------
// Deterministic (no atomics), two launches.  Stage 1: block b of 256 threads owns the GRAD_NORM_F4 * 256 16-byte elements from
// b * GRAD_NORM_F4 * 256 on; thread t reads elements t, t + 256, ... (all loads in flight before the first use), squares and
// adds them into one fp32 accumulator per vector component -- GRAD_NORM_F4 serial additions -- adds the four components as
// (0 + 1) + (2 + 3), and the block sums its 256 values in a fixed tree: xor-shuffles over the 64 lanes (6 levels), then the
// four waves through LDS as (w0 + w1) + (w2 + w3).  The block's sum leaves fp32 here: part[b] is a double.
// Stage 2: ONE block; thread t adds part[t], part[t + 256], ... in double, in that order, the 256 sums are folded in LDS in a
// fixed halving tree, and thread 0 writes sqrtf of the total as one float.
// Elements past n4 (the last block's tail) read as zero.  The engine's padding inside the arena holds exact zeros.
__global__ void __launch_bounds__(256) grad_sqsum_kernel(const float* __restrict__ g, int64_t n4, double* __restrict__ part,
                                                         const int* __restrict__ skip)
{
    if (skip && *skip) return;
    __shared__ float wsum[4];
    const int64_t base = (int64_t)blockIdx.x * (GRAD_NORM_F4 * 256) + threadIdx.x;
    f32x4 v[GRAD_NORM_F4];
#pragma unroll
    for (int j = 0; j < GRAD_NORM_F4; ++j) {
        const int64_t i = base + (int64_t)j * 256;
        v[j] = i < n4 ? reinterpret_cast<const f32x4*>(g)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < GRAD_NORM_F4; ++j) acc = acc + v[j] * v[j];
    float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (double)((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
}
__global__ void __launch_bounds__(256) grad_norm_final_kernel(const double* __restrict__ part, int nparts, float* __restrict__ norm,
                                                              const int* __restrict__ skip)
{
    if (skip && *skip) return;
    __shared__ double sm[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *norm = sqrtf((float)sm[0]);
}
int grad_norm_parts(int64_t n) { return cdiv(n / 4, (int64_t)GRAD_NORM_F4 * 256); }
void k_grad_norm(const float* g, int64_t n, double* part, float* norm, hipStream_t s, const int* skip)
{
    const int nparts = grad_norm_parts(n);
    hipLaunchKernelGGL(grad_sqsum_kernel, dim3(nparts), dim3(256), 0, s, g, n / 4, part, skip);
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, s, part, nparts, norm, skip);
}

// ---------------------------------------------------------------- clips --------
// torch.nn.utils.clip_grad_norm_: g *= min(1, max_norm / (norm + 1e-6)), the coefficient formed in fp32 from the device word;
// the multiply always happens and a non-finite norm propagates (a NaN coefficient is not clamped, like torch.clamp).
__global__ void grad_clip_norm_kernel(float* __restrict__ g, int64_t n4, const float* __restrict__ norm, float max_norm,
                                      const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    float c = max_norm / (*norm + 1e-6f);
    c = c > 1.f ? 1.f : c;
    reinterpret_cast<f32x4*>(g)[i] = reinterpret_cast<const f32x4*>(g)[i] * c;
}
void k_grad_clip_norm(float* g, int64_t n, const float* norm, float max_norm, hipStream_t s, const int* skip)
{
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(grad_clip_norm_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, s, g, n4, norm, max_norm, skip);
}

// torch.nn.utils.clip_grad_value_: g = clamp(g, -clip, clip); a NaN stays a NaN
__global__ void grad_clip_value_kernel(float* __restrict__ g, int64_t n4, float clip, const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    f32x4 x = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = x[k] < -clip ? -clip : (x[k] > clip ? clip : x[k]);
    reinterpret_cast<f32x4*>(g)[i] = x;
}
void k_grad_clip_value(float* g, int64_t n, float clip, hipStream_t s, const int* skip)
{
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(grad_clip_value_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, s, g, n4, clip, skip);
}

// ------------------------------------------- parameter groups, frozen entries --------
// The three steps again, over the parameter chunks of the engine's entry / chunk table (arena_table.h) instead of the flat
// arena: one block of 256 threads per chunk of <= FM_DIST_CHUNK floats of ONE state entry, whose parameter group the block
// fetches once from the launch's own argument block (OptSel: four bits per entry).  An entry nobody steps -- in no group, or
// frozen -- costs its blocks one kernel-argument read: they return before any load.  The hyper-parameters are an argument
// array of OPT_MAX_GROUPS structs holding what the single-group launchers pass to their kernels, formed the same way on the host.
//
// arena_walk has the boundary rule (whole quads read, own floats written).  Floats outside every entry (the gaps between
// matrices and vectors, a padded BatchNorm vector's tail) are touched by nobody and stay zero; padding inside an entry's span
// (padded input channels and taps, the packed stem's row tails) is stepped with its entry and stays zero under all three
// rules (zero weight, zero gradient: DESIGN.md section 1's padding note).
//
// The arithmetic per element is the rule's update(), the one the flat steps call.
template <class R, class Args>
__global__ void __launch_bounds__(256) opt_groups_kernel(const R r, const Args a, const ArenaChunk* __restrict__ chunks, const OptSel sel,
                                                         const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const ArenaChunk ch = chunks[blockIdx.x];
    const unsigned gi = opt_sel_get(sel, ch.ent);
    if (gi >= OPT_MAX_GROUPS) return;             // in no group, or frozen: before any load
    arena_walk(r, ch, a.hp[gi]);
}
__global__ void __launch_bounds__(256) sgd_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                         const OptSgdArgs a, const ArenaChunk* __restrict__ chunks, const OptSel sel,
                                                         const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const ArenaChunk ch = chunks[blockIdx.x];
    const unsigned gi = opt_sel_get(sel, ch.ent);
    if (gi >= OPT_MAX_GROUPS) return;
    const int mode = a.hp[gi].mode;
    if (mode == 0) arena_walk(SgdRule<0>{p, g, buf}, ch, a.hp[gi]);
    else if (mode == 1) arena_walk(SgdRule<1>{p, g, buf}, ch, a.hp[gi]);
    else arena_walk(SgdRule<2>{p, g, buf}, ch, a.hp[gi]);
}

void k_adam_groups(float* p, const float* g, float* m, float* v, const ArenaChunk* chunks, int n_chunks, const OptSel& sel,
                   const OptAdamArgs& a, hipStream_t s, const int* skip)
{
    hipLaunchKernelGGL((opt_groups_kernel<AdamRule, OptAdamArgs>), dim3(n_chunks), dim3(256), 0, s, AdamRule{{p, g, m, v}}, a, chunks, sel, skip);
}
void k_adamw_groups(float* p, const float* g, float* m, float* v, const ArenaChunk* chunks, int n_chunks, const OptSel& sel,
                    const OptAdamWArgs& a, hipStream_t s, const int* skip)
{
    hipLaunchKernelGGL((opt_groups_kernel<AdamWRule, OptAdamWArgs>), dim3(n_chunks), dim3(256), 0, s, AdamWRule{{p, g, m, v}}, a, chunks, sel, skip);
}
void k_sgd_groups(float* p, const float* g, float* buf, const ArenaChunk* chunks, int n_chunks, const OptSel& sel,
                  const OptSgdArgs& a, hipStream_t s, const int* skip)
{
    hipLaunchKernelGGL(sgd_groups_kernel, dim3(n_chunks), dim3(256), 0, s, p, g, buf, a, chunks, sel, skip);
}

// ------------------------------------------------- gradient accumulator --------
// The accumulator of the autograd path (fm_backward_grads): acc = g when the accumulator is empty (a copy, so one backward
// after fm_zero_grad holds exactly the fused path's gradients), acc += g after it; one streaming float4 pass over the arena
__global__ void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, int64_t n4, int copy,
                                       const int* __restrict__ skip)
{
    if (skip && *skip) return;      // a lost stream-K part poisoned g: the accumulator stays as it is
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
        reinterpret_cast<f32x4*>(acc)[i] = copy ? gg : reinterpret_cast<const f32x4*>(acc)[i] + gg;
    }
}
void k_grad_accumulate(float* acc, const float* g, int64_t n, bool copy, hipStream_t s, const int* skip)
{
    const int64_t n4 = n / 4;     // engine pads the parameter arena to a multiple of 4
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, s, acc, g, n4, copy ? 1 : 0, skip);
}

// k_grad_accumulate under a mask, over the same table with the same boundary rule: sel = 0 marks a trainable entry (acc = g or
// acc += g, the flat kernel's one addition), anything else a frozen one, whose span becomes exact zeros in both forms -- whatever
// e->grad holds there (a skipped weight gradient leaves it stale).
__global__ void __launch_bounds__(256) grad_accumulate_masked_kernel(float* __restrict__ acc, const float* __restrict__ g,
                                                                     const ArenaChunk* __restrict__ chunks, const OptSel sel, int copy,
                                                                     const int* __restrict__ skip)
{
    if (skip && *skip) return;
    const ArenaChunk ch = chunks[blockIdx.x];
    const bool frozen = opt_sel_get(sel, ch.ent) != 0u;
    const int64_t begin = ch.begin, end = begin + ch.len;
    for (int64_t o = (begin & ~(int64_t)3) + 4 * (int64_t)threadIdx.x; o < end; o += 1024) {
        f32x4 r = {0.f, 0.f, 0.f, 0.f};
        if (!frozen) {
            const f32x4 gg = *reinterpret_cast<const f32x4*>(g + o);
            r = copy ? gg : *reinterpret_cast<const f32x4*>(acc + o) + gg;
        }
        store_own(acc, o, begin, end, r);
    }
}
void k_grad_accumulate_masked(float* acc, const float* g, const ArenaChunk* chunks, int n_chunks, const OptSel& sel, bool copy,
                              hipStream_t s, const int* skip)
{
    hipLaunchKernelGGL(grad_accumulate_masked_kernel, dim3(n_chunks), dim3(256), 0, s, acc, g, chunks, sel, copy ? 1 : 0, skip);
}
